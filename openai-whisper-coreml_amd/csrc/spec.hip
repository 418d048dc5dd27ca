// spec.hip -- the kernels of a speculative decode round (wm_transcribe_mel_speculative) around the
// target's verify step: the draft's adoption of the first token, the staging of a round's proposals (with the replay of the
// timestamp rules along them), the close of the verify step's rows (accept) and the group's lockstep cut (commit).
// A row's close is the one-wave close of panel_rows.h (the arg-max close of dec_kernels.hip argmax_embed_body<true>: the same
// calls into dec_close.h), so winner, tie order, forced timestamps and log-prob are the plain step's; the accept kernel itself
// holds only the window's acceptance count.  The committed-state load and store and the stage loop are panel_rows.h's too.
#include "panel_rows.h"
#include "spec_round.h"

namespace {

// The draft adopts the target's first generated token (position n_prompt of both token buffers): its own choice there is
// overwritten, its timestamp-rule state is the initial one advanced by the target's token.  One thread per window.
__global__ void spec_adopt_kernel(WmSpecDev sp, int G, int n_prompt) {
    const int c = threadIdx.x;
    if (c >= G) return;
    const int tok = sp.tseq[n_prompt * G + c];
    sp.dseq[n_prompt * G + c] = tok;
    sp.stats[c * 4 + 0] = 0; sp.stats[c * 4 + 1] = 0; sp.stats[c * 4 + 2] = 0; sp.stats[c * 4 + 3] = 0;
    int hs[4];
    if (sp.tts.rng) {   // the target's committed state: what its first close left
        const int4 r = panel_state_load(sp.tts.hist, sp.tts.rng, c, hs);
        panel_state_store(sp.chist, sp.crng, c, hs, r);
    }
    if (sp.dts.rng) {   // (ts_init_kernel's history, advanced by the adopted token)
        hs[0] = 0; hs[1] = 0; hs[2] = 1; hs[3] = -1;
        const int4 r = ts_advance(sp.dts, hs, tok);
        panel_state_store(sp.dts.hist, sp.dts.rng, c, hs, r);
        panel_state_store(sp.dchist, sp.dcrng, c, hs, r);
    }
}

// The proposals of a round of width w go into the TARGET's token buffer behind its last token: d[s - 1] of window c at
// position pos + s (the draft's own tokens, or the debug script's).  Row (c, s) of the verify step needs the timestamp-rule
// ranges as they stand after d[0 .. s): replayed from the window's committed state into the rows' slots.  One thread per window.
__global__ void spec_stage_kernel(WmSpecDev sp, int G, int w, int n_prompt, int n_ctx) {
    const int c = threadIdx.x;
    if (c >= G) return;
    const int pos = *sp.tpos;
    int hs[4] = {0, 0, 0, 0};
    int4 rng = make_int4(0, 0, 0, 0);
    if (sp.tts.rng) rng = panel_state_load(sp.chist, sp.crng, c, hs);
    panel_stage_window(sp.tts, sp.tseq, G, c, w, pos, n_ctx, hs, rng, [&](int, int p) {
        const int gi = p - n_prompt;   // the proposal is generated token gi
        const int tok = (sp.script && gi >= 0 && gi < sp.max_new) ? sp.script[(long)c * sp.max_new + gi] : sp.dseq[p * G + c];
        return tok < 0 ? 0 : (tok >= sp.n_vocab ? sp.n_vocab - 1 : tok);
    });
}

// ACCEPT.  One workgroup per window, wave s closes row (c, s) = row c * w + s of the verify step.  Then the window's leading rows
// whose winner equals the proposal are counted: a_c, and n_c = a_c + 1 tokens are the target's own.
__global__ __launch_bounds__(512) void spec_accept_kernel(const unsigned long long *__restrict__ tilemax, int n_tiles, int G, int w,
                                                          WmSpecDev sp, WmXDev xd, int fallback_tok) {
    __shared__ float seg_s[8][16][4];
    __shared__ int tok_s[8];
    __shared__ float lp_s[8];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, c = blockIdx.x;
    const WmTsDev &ts = sp.tts;
    unsigned long long key = 0ull;
    if (s < w) key = panel_close_begin(tilemax, xd, c * w + s, n_tiles, lane, seg_s[s]);   // wave-uniform
    __syncthreads();   // (the barrier between the halves of the close: panel_rows.h)
    if (s < w) {   // wave-uniform
        Lse lt;
        const PanelRowClose r = panel_close_end(ts, xd, c * w + s, n_tiles, lane, key, seg_s[s], lt, fallback_tok);
        if (lane == 0) {
            tok_s[s] = r.tok;
            lp_s[s] = r.lp;
        }
    }
    __syncthreads();
    if (threadIdx.x < w) {
        sp.wtok[c * w + threadIdx.x] = tok_s[threadIdx.x];
        sp.wlp[c * w + threadIdx.x] = lp_s[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        const int pos = *sp.tpos;
        int a = 0;
        while (a < w - 1 && tok_s[a] == sp.tseq[(pos + 1 + a) * G + c]) ++a;
        sp.acc[c] = a;
    }
}

// COMMIT: the lockstep cut and what follows from it.  ONE workgroup, thread c owns window c.  n = the fewest tokens a live window
// could keep; every live window writes its first n verified tokens and their log-probs (up to its stopping token: spec_round.h),
// commits the timestamp-rule state behind them and updates its stop state and statistics; a frozen window writes padding, as a
// finished row of the plain call does.  Then both models' positions advance by n, the draft's token buffer takes the target's
// last token and the draft's timestamp-rule state is rebuilt from its committed one along the kept tokens.
__global__ __launch_bounds__(WM_DEC_MAXB) void spec_commit_kernel(WmSpecDev sp, WmXDev xd, WmStopDev stop, int G, int w, int n_prompt,
                                                                  int n_ctx) {
    __shared__ int red_s[WM_DEC_MAXB];
    const int c = threadIdx.x;
    const int pos = *sp.tpos;
    const bool mine = c < G;
    const bool live = mine && stop.done[c] == 0;
    const int a = mine ? sp.acc[c] : 0;
    const int g0 = pos + 1 - n_prompt;   // generated index of the round's first token
    int eot_at = -1, left = 0;
    if (live) {   // among the window's own a + 1 tokens
        if (stop.eot >= 0)
            for (int i = 0; i <= a && i < w && eot_at < 0; ++i)
                if (sp.wtok[c * w + i] == stop.eot) eot_at = i;
        left = (stop.budget && stop.budget[c] < sp.max_new ? stop.budget[c] : sp.max_new) - g0;
    }
    red_s[c] = live ? wm_spec_window_ask(a, eot_at, left) : WM_SPEC_NO_CUT;
    __syncthreads();
    for (int o = WM_DEC_MAXB / 2; o > 0; o >>= 1) {   // a minimum: any order, same value
        if (c < o) red_s[c] = red_s[c + o] < red_s[c] ? red_s[c + o] : red_s[c];
        __syncthreads();
    }
    const int asked = red_s[0];
    __syncthreads();
    red_s[c] = live ? 1 : 0;
    __syncthreads();
    for (int o = WM_DEC_MAXB / 2; o > 0; o >>= 1) {
        if (c < o) red_s[c] += red_s[c + o];
        __syncthreads();
    }
    // nobody is live (a round enqueued ahead of the host's last look): nothing moves; every live window finishes: the whole width
    int n = red_s[0] == 0 ? 0 : (asked < w ? asked : w);
    __syncthreads();
    if (pos + n >= n_ctx) n = n_ctx - 1 - pos > 0 ? n_ctx - 1 - pos : 0;   // (never: the host narrows the last rounds)
    int now_live = 0;
    if (mine) {
        int m = 0, stops = 0, acc = 0, kept = 0;
        if (live) wm_spec_window_cut(n, a, eot_at, left, &m, &stops, &acc, &kept);
        int hs[4] = {0, 0, 0, 0};
        int4 rng = make_int4(0, 0, 0, 0);
        if (sp.tts.rng) rng = panel_state_load(sp.chist, sp.crng, c, hs);
        for (int i = 0; i < n; ++i) {
            const int tok = i < m ? sp.wtok[c * w + i] : stop.pad_tok;
            const float lp = i < m ? sp.wlp[c * w + i] : 0.f;
            sp.tseq[(pos + 1 + i) * G + c] = tok;
            if (g0 + i >= 0 && g0 + i < sp.max_new) xd.logprob[(long)(g0 + i) * G + c] = lp;
            if (sp.tts.rng && i < m) rng = ts_advance(sp.tts, hs, tok);
        }
        if (sp.tts.rng && m > 0) panel_state_store(sp.chist, sp.crng, c, hs, rng);
        if (live) {
            if (stops) stop.done[c] = 1;
            now_live = stops ? 0 : 1;
            sp.stats[c * 4 + 0] += 1;
            sp.stats[c * 4 + 1] += w - 1;
            sp.stats[c * 4 + 2] += acc;
            sp.stats[c * 4 + 3] += kept;
        }
        // the draft: the token it continues from, and its rules' state behind the n tokens the group advanced by
        if (n > 0) sp.dseq[(pos + n) * G + c] = sp.tseq[(pos + n) * G + c];
        if (sp.dts.rng) {
            int dh[4];
            int4 dr = panel_state_load(sp.dchist, sp.dcrng, c, dh);
            for (int i = 0; i < n; ++i) dr = ts_advance(sp.dts, dh, sp.tseq[(pos + 1 + i) * G + c]);
            panel_state_store(sp.dts.hist, sp.dts.rng, c, dh, dr);
            panel_state_store(sp.dchist, sp.dcrng, c, dh, dr);
        }
    }
    red_s[c] = now_live;
    __syncthreads();
    for (int o = WM_DEC_MAXB / 2; o > 0; o >>= 1) {
        if (c < o) red_s[c] += red_s[c + o];
        __syncthreads();
    }
    if (c == 0) {
        *sp.tpos = pos + n;
        *sp.dpos = pos + n;
        *stop.n_live = red_s[0];
        sp.round[0] = red_s[0];
        sp.round[1] = pos + n;
    }
}

}  // namespace

int wm_spec_adopt(wm_ctx *draft, const WmSpecDev &sp, int G, int n_prompt) {
    WM_REQUIRE(G >= 1 && G <= WM_DEC_MAXB, WM_ERR_INVALID, "spec_adopt: %d windows", G);
    WmProfScope ps(&draft->prof, "spec_adopt", draft->stream);
    spec_adopt_kernel<<<1, WM_DEC_MAXB, 0, draft->stream>>>(sp, G, n_prompt);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_spec_stage(wm_ctx *ctx, const WmSpecDev &sp, int G, int w, int n_prompt, int n_ctx) {
    WM_TRY(wm_panel_shape_check(G, w, "spec_stage"));
    WmProfScope ps(&ctx->prof, "spec_stage", ctx->stream);
    spec_stage_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(sp, G, w, n_prompt, n_ctx);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_spec_accept(wm_ctx *ctx, const unsigned long long *tilemax, int n_tiles, const WmSpecDev &sp, const WmXDev &xd,
                   const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx, int fallback_tok) {
    WM_TRY(wm_panel_shape_check(G, w, "spec_accept"));
    WM_REQUIRE(xd.par && stop.done, WM_ERR_STATE, "spec_accept: needs the extended decode and the stop state");
    WmProfScope ps(&ctx->prof, "spec_accept", ctx->stream);
    spec_accept_kernel<<<G, 512, 0, ctx->stream>>>(tilemax, n_tiles, G, w, sp, xd, fallback_tok);
    WM_HIP(hipGetLastError());
    return wm_spec_commit(ctx, sp, xd, stop, G, w, n_prompt, n_ctx);
}

// the second launch of wm_spec_accept (which the product always makes through it; alone: the debug library's kernel tests)
int wm_spec_commit(wm_ctx *ctx, const WmSpecDev &sp, const WmXDev &xd, const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx) {
    WM_TRY(wm_panel_shape_check(G, w, "spec_commit"));
    WM_REQUIRE(xd.logprob && stop.done, WM_ERR_STATE, "spec_commit: needs the extended decode and the stop state");
    spec_commit_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(sp, xd, stop, G, w, n_prompt, n_ctx);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
