// given_panel.hip -- given tokens in panels (wm_set_given_panel): the kernels around the panel step of a
// round that scores w positions of every window's given text at once.  STAGE puts the round's inputs into the token buffer and
// replays the timestamp rules along them into the rows' range slots (panel_rows.h's stage loop, which spec_stage_kernel runs
// from a draft and this one from the table); CLOSE does, per row of the step and by ONE wave, what given_tokens_kernel (given.hip)
// and then the arg-max close (argmax_embed_body<true>, spec_accept_kernel) do for a row of the plain step -- the one-wave close of
// panel_rows.h around stored_row.h's admissibility test and hand-over, so the case table at row_hand_over applies unchanged;
// COMMIT applies the stop bookkeeping of the plain close along a window's w tokens and, behind the last round, puts the [G]
// layout of the step path back.  Vector stores and shared-memory reductions only; nothing atomic.
#include "model.h"
#include "panel_rows.h"
#include "stored_row.h"

namespace {

// the given token of window c at generated index gi, or -1 where the table has none
__device__ __forceinline__ int panel_given(const WmGivenPar &par, int c, int gi) {
    if (gi < 0 || gi >= par.stride || gi >= par.lens[c]) return -1;
    return par.tok[(long)c * par.stride + gi];
}

// STAGE.  One workgroup, thread c owns window c.
__global__ __launch_bounds__(WM_DEC_MAXB) void given_panel_stage_kernel(WmGivenPanelDev gp, int pad_tok, int G, int w, int n_prompt,
                                                                        int n_ctx, int first) {
    const int c = threadIdx.x;
    const bool mine = c < G;
    const WmTsDev &ts = gp.ts;
    const int pos = *gp.pos, g0 = pos + 1 - n_prompt;
    int hs[4] = {0, 0, 0, 0};
    int4 rng = make_int4(0, 0, 0, 0);
    // the committed state: the step path's own [G] slots in front of the first round, the side area after
    if (mine && ts.rng) rng = panel_state_load(first ? ts.hist : gp.chist, first ? ts.rng : gp.crng, c, hs);
    __syncthreads();   // every window's [G] slot is read: the rows' slots [G x w], which overlap them, may be written
    if (!mine) return;
    if (ts.rng && first) panel_state_store(gp.chist, gp.crng, c, hs, rng);
    const WmGivenPar par = *gp.par;
    panel_stage_window(ts, gp.seq, G, c, w, pos, n_ctx, hs, rng, [&](int s, int) {
        const int tok = panel_given(par, c, g0 + s - 1);   // the input of row (c, s) is generated token g0 + s - 1
        return (tok < 0 || tok >= gp.n_vocab) ? pad_tok : tok;   // (a window its budget has finished by then: any valid id)
    });
}

// CLOSE.  One workgroup per window, wave s closes row (c, s) = row c * w + s of the panel step.
__global__ __launch_bounds__(512) void given_panel_close_kernel(const float *__restrict__ logits, long ldo, int V, unsigned long long *tilemax,
                                                                int n_tiles, int w, int n_prompt, WmGivenPanelDev gp, WmXDev xd,
                                                                const unsigned *__restrict__ mask, int fallback_tok) {
    __shared__ float seg_s[8][16][4];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, c = blockIdx.x;
    const WmTsDev &ts = gp.ts;
    const bool active = s < w;   // wave-uniform
    const int b = c * w + (active ? s : 0);
    const long rb = (long)b * n_tiles;
    const int gi = *gp.pos + 1 - n_prompt + s;
    unsigned long long key = 0ull;
    if (active) key = panel_close_begin(tilemax, xd, b, n_tiles, lane, seg_s[s]);
    __syncthreads();   // (the barrier between the halves of the close: panel_rows.h)
    Lse lt{-1e30f, 0.f};
    const float(*seg)[4] = seg_s[s];   // (null once lt holds the row's total)
    if (active) {
        const int tok = panel_given(*gp.par, c, gi);
        if (tok >= 0 && tok < V) {   // given_tokens_kernel's steps for this row (wave-uniform)
            const RowChoice c0 = panel_close_choose(ts, b, n_tiles, lane, key, seg, lt);
            seg = nullptr;
            if (row_best_value(c0, lt) > -1e30f) {   // (nothing admissible: the close below takes its existing path -- the fallback token, -inf)
                // (no ban row; never the first generated position -- the ordinary step takes it -- so no first-position offset)
                const RowAdmit adm = row_admit_set(V, ts, mask, 0, nullptr, 0, b, 0, 0, c0.forced);
                const float v = logits[(long)b * ldo + tok];
                const float val = (row_admits(adm, tok) && v > -INFINITY) ? v : -INFINITY;   // (NaN: not admissible)
                // the hand-over: only the given id is left in the row's keys.  Every read of them above has been consumed (c0).
                row_hand_over(ts, tilemax, rb, n_tiles, c0.forced, argmax_key(val, tok), lane, 64);
                if (lane == 0) xd.win[row_win_slot(ts, rb, tok)] = val;
            }
        }
    }
    __syncthreads();   // the hand-over's stores are behind this barrier: the row's keys are read again
    if (active) {   // the arg-max close of the row on what the hand-over left (a given row's total stands: seg is null)
        key = panel_row_key(tilemax + rb, n_tiles, lane);
        const PanelRowClose r = panel_close_end(ts, xd, b, n_tiles, lane, key, seg, lt, fallback_tok);
        if (lane == 0) {
            gp.wtok[b] = r.tok;
            gp.wlp[b] = r.lp;
        }
    }
}

// COMMIT.  One workgroup, thread c owns window c.
__global__ __launch_bounds__(WM_DEC_MAXB) void given_panel_commit_kernel(WmGivenPanelDev gp, WmXDev xd, WmStopDev stop, int G, int w,
                                                                         int n_prompt, int last) {
    const int c = threadIdx.x;
    const WmTsDev &ts = gp.ts;
    const int pos = *gp.pos, g0 = pos + 1 - n_prompt;
    if (c < G) {
        bool live = !stop.done || stop.done[c] == 0;
        int hs[4] = {0, 0, 0, 0};
        int4 rng = make_int4(0, 0, 0, 0);
        if (ts.rng) rng = panel_state_load(gp.chist, gp.crng, c, hs);
        for (int i = 0; i < w; ++i) {
            const int gi = g0 + i;
            int tok = stop.pad_tok;   // finished earlier: padding, log-prob 0 (the plain close's finished row)
            float lp = 0.f;
            if (live) {
                tok = gp.wtok[c * w + i];
                lp = gp.wlp[c * w + i];
                if (ts.rng) rng = ts_advance(ts, hs, tok);
                // this token is the window's last: the plain close's test
                if (stop.done && ((stop.eot >= 0 && tok == stop.eot) || (stop.budget && gi + 1 >= stop.budget[c]))) {
                    live = false;
                    stop.done[c] = 1;
                }
            }
            gp.seq[(pos + 1 + i) * G + c] = tok;
            if (gi >= 0 && gi < gp.max_new) xd.logprob[(long)gi * G + c] = lp;
        }
        if (ts.rng) {
            panel_state_store(gp.chist, gp.crng, c, hs, rng);
            if (last) panel_state_store(ts.hist, ts.rng, c, hs, rng);   // the [G] layout of the step path (nobody reads the rows' slots any more)
        }
    }
    __syncthreads();   // the done flags of every window are written
    if (stop.done && threadIdx.x < 64) live_list_rebuild(stop, G, threadIdx.x, [&](int r) { return stop.done[r] == 0; });
    if (c == 0) *gp.pos = pos + w;
}

}  // namespace

int wm_given_panel_stage(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx, bool first) {
    WM_TRY(wm_panel_shape_check(G, w, "given_panel_stage"));
    WM_REQUIRE(gp.seq && gp.pos && gp.par && (!gp.ts.rng || (gp.chist && gp.crng && gp.ts.hist)), WM_ERR_INVALID, "given_panel_stage: bad state");
    WmProfScope ps(&ctx->prof, "given_panel_stage", ctx->stream);
    given_panel_stage_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(gp, stop.pad_tok, G, w, n_prompt, n_ctx, first ? 1 : 0);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_given_panel_close(wm_ctx *ctx, const WmStoredRows &r, const WmGivenPanelDev &gp, int G, int w, int fallback_tok, bool last) {
    WM_TRY(wm_panel_shape_check(G, w, "given_panel_close"));
    WM_TRY(wm_stored_rows_check(r, "given_panel_close", true));
    WM_REQUIRE(r.rows == G * w && r.n_vocab == gp.n_vocab && r.ts.rng == gp.ts.rng && r.pos_ptr == gp.pos && gp.par && gp.wtok && gp.wlp,
               WM_ERR_INVALID, "given_panel_close: the rows are not the round's %d x %d, or the group has no table", G, w);
    {
        WmProfScope ps(&ctx->prof, "given_panel_close", ctx->stream);
        given_panel_close_kernel<<<G, 512, 0, ctx->stream>>>(r.logits, r.ldo, r.n_vocab, r.tilemax, (r.n_vocab + 15) / 16, w, r.n_prompt, gp,
                                                             r.xd, r.mask, fallback_tok);
        WM_HIP(hipGetLastError());
    }
    return wm_given_panel_commit(ctx, gp, r.xd, r.stop, G, w, r.n_prompt, last);
}

// the second launch of wm_given_panel_close (which the product always makes through it; alone: the debug library's kernel tests)
int wm_given_panel_commit(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmXDev &xd, const WmStopDev &stop, int G, int w, int n_prompt,
                          bool last) {
    WM_TRY(wm_panel_shape_check(G, w, "given_panel_commit"));
    WM_REQUIRE(xd.logprob && gp.seq && gp.pos && gp.wtok && gp.wlp && (!gp.ts.rng || (gp.chist && gp.crng && gp.ts.hist)), WM_ERR_INVALID,
               "given_panel_commit: needs the extended decode and the round's state");
    WM_REQUIRE(!stop.done || (stop.live_rows && stop.n_live), WM_ERR_INVALID, "given_panel_commit: incomplete stop state");
    WmProfScope ps(&ctx->prof, "given_panel_commit", ctx->stream);
    given_panel_commit_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(gp, xd, stop, G, w, n_prompt, last ? 1 : 0);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
