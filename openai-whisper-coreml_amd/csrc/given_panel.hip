// given_panel.hip -- given tokens in panels (wm_set_given_panel): the kernels around the panel step of a
// round that scores w positions of every window's given text at once.  STAGE puts the round's inputs into the token buffer and
// replays the timestamp rules along them into the rows' range slots (spec_stage_kernel's job, from the table instead of a
// draft); CLOSE does, per row of the step and by ONE wave, what given_tokens_kernel (given.hip) and then the arg-max close
// (argmax_embed_body<true>, spec_accept_kernel) do for a row of the plain step -- every order-sensitive piece is a call into
// dec_close.h, the admissibility test is row_list.h's, so the case table of given.hip applies unchanged; COMMIT applies the stop
// bookkeeping of the plain close along a window's w tokens and, behind the last round, puts the [G] layout of the step path back.
// Vector stores and shared-memory reductions only; nothing atomic.
#include "dec_close.h"
#include "model.h"
#include "row_list.h"

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
    if (mine && ts.rng) {   // the committed state: the step path's own [G] slots in front of the first round, the side area after
        const int4 h = *(const int4 *)((first ? ts.hist : gp.chist) + c * 4);
        hs[0] = h.x; hs[1] = h.y; hs[2] = h.z; hs[3] = h.w;
        rng = *(const int4 *)((first ? ts.rng : gp.crng) + c * 4);
    }
    __syncthreads();   // every window's [G] slot is read: the rows' slots [G x w], which overlap them, may be written
    if (!mine) return;
    if (ts.rng) {
        if (first) {
            *(int4 *)(gp.chist + c * 4) = make_int4(hs[0], hs[1], hs[2], hs[3]);
            *(int4 *)(gp.crng + c * 4) = rng;
        }
        *(int4 *)(ts.rng + (c * w) * 4) = rng;
    }
    const WmGivenPar par = *gp.par;
    for (int s = 1; s < w; ++s) {
        const int p = pos + s;
        if (p >= n_ctx) break;
        int tok = panel_given(par, c, g0 + s - 1);   // the input of row (c, s) is generated token g0 + s - 1
        if (tok < 0 || tok >= gp.n_vocab) tok = pad_tok;   // (a window its budget has finished by then: any valid id)
        gp.seq[p * G + c] = tok;
        if (ts.rng) *(int4 *)(ts.rng + (c * w + s) * 4) = ts_advance(ts, hs, tok);
    }
}

// the row's best text key over its tiles, every lane holding it
__device__ __forceinline__ unsigned long long panel_row_key(const unsigned long long *row, int n_tiles, int lane) {
    unsigned long long key = 0ull;
    for (int t = lane; t < n_tiles; t += 64) {
        const unsigned long long k = row[t];
        key = k > key ? k : key;
    }
    return key_max_xor<64>(key);
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
    if (active) {
        key = panel_row_key(tilemax + rb, n_tiles, lane);
        lse_row_segments(xd, rb, n_tiles, false, 0, 1, lane, seg_s[s]);
    }
    __syncthreads();   // lane 0 wrote the row's 16 segments, lanes 0 .. 15 read them: the barrier argmax_embed_body has here
    Lse lt{-1e30f, 0.f}, la{-1e30f, 0.f};
    if (active) {
        lse_row_total(seg_s[s], lane, lt, la);
        const int tok = panel_given(*gp.par, c, gi);
        if (tok >= 0 && tok < V) {   // given_tokens_kernel's steps for this row (wave-uniform)
            const RowChoice c0 = row_choose(ts, b, n_tiles, lane, key, lt.m);
            const float vmax = c0.forced ? c0.lts.m : fmaxf(lt.m, c0.lts.m);
            if (vmax > -1e30f) {   // (nothing admissible: the close below takes its existing path -- the fallback token, -inf)
                RowAdmit adm;
                adm.V = V;
                adm.rng = make_int4(0, V, 0, 0);
                if (ts.rng) adm.rng = *(const int4 *)(ts.rng + b * 4);
                adm.forced = c0.forced;
                adm.mrow = mask;   // (never the first generated position: the ordinary step takes it)
                adm.brow = nullptr;
                const float v = logits[(long)b * ldo + tok];
                const float val = (row_admits(adm, tok) && v > -INFINITY) ? v : -INFINITY;   // (NaN: not admissible)
                const unsigned long long win = argmax_key(val, tok);
                // the hand-over: only the given id is left in the row's keys.  Every read of them above has been consumed (c0).
                const int wt = tok >> 4;
                const int side = (ts.rng && tok >= ts.ts_begin) ? 1 : 0;
                const int t_first = ts.ts_begin >> 4;
                for (int t = lane; t < n_tiles; t += 64) {
                    tilemax[rb + t] = (side == 0 && t == wt) ? win : ((side == 1 && !c0.forced && t == 0) ? 1ull : 0ull);
                    if (ts.rng && t >= t_first) ts.key_ts[rb + t] = (side == 1 && t == wt) ? win : 0ull;
                }
                if (lane == 0) xd.win[(rb + wt) * 2 + side] = val;
            }
        }
    }
    __syncthreads();   // the hand-over's stores are behind this barrier: the row's keys are read again
    if (active) {   // the arg-max close of the row, as spec_accept_kernel has it
        key = panel_row_key(tilemax + rb, n_tiles, lane);
        const RowChoice ch = row_choose(ts, b, n_tiles, lane, key, lt.m);
        if (lane == 0) {
            gp.wtok[b] = ch.key ? argmax_key_index(ch.key) : fallback_tok;
            gp.wlp[b] = row_logprob(ts, xd, b, n_tiles, ch, lt);
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
        if (ts.rng) {
            const int4 h = *(const int4 *)(gp.chist + c * 4);
            hs[0] = h.x; hs[1] = h.y; hs[2] = h.z; hs[3] = h.w;
            rng = *(const int4 *)(gp.crng + c * 4);
        }
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
            *(int4 *)(gp.chist + c * 4) = make_int4(hs[0], hs[1], hs[2], hs[3]);
            *(int4 *)(gp.crng + c * 4) = rng;
            if (last) {   // the [G] layout of the step path (nobody reads the rows' slots any more)
                *(int4 *)(ts.hist + c * 4) = make_int4(hs[0], hs[1], hs[2], hs[3]);
                *(int4 *)(ts.rng + c * 4) = rng;
            }
        }
    }
    __syncthreads();   // the done flags of every window are written
    if (stop.done && threadIdx.x < 64) live_list_rebuild(stop, G, threadIdx.x, [&](int r) { return stop.done[r] == 0; });
    if (c == 0) *gp.pos = pos + w;
}

int panel_check(int G, int w, const char *what) {
    WM_REQUIRE(G >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && G * w <= WM_DEC_MAXB, WM_ERR_INVALID, "%s: %d windows x %d rows", what, G, w);
    return WM_OK;
}

}  // namespace

int wm_given_panel_stage(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx, bool first) {
    WM_TRY(panel_check(G, w, "given_panel_stage"));
    WM_REQUIRE(gp.seq && gp.pos && gp.par && (!gp.ts.rng || (gp.chist && gp.crng && gp.ts.hist)), WM_ERR_INVALID, "given_panel_stage: bad state");
    WmProfScope ps(&ctx->prof, "given_panel_stage", ctx->stream);
    given_panel_stage_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(gp, stop.pad_tok, G, w, n_prompt, n_ctx, first ? 1 : 0);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_given_panel_close(wm_ctx *ctx, const float *logits, long ldo, unsigned long long *tilemax, int n_tiles, const WmGivenPanelDev &gp,
                         const WmXDev &xd, const WmStopDev &stop, const unsigned *mask, int mask_words, int G, int w, int n_prompt,
                         int fallback_tok, bool last) {
    WM_TRY(panel_check(G, w, "given_panel_close"));
    WM_REQUIRE(logits && tilemax && xd.par && xd.txt && xd.win && gp.par && gp.wtok && gp.wlp && gp.pos, WM_ERR_INVALID,
               "given_panel_close: needs the extended decode and the group's table");
    WM_REQUIRE(gp.n_vocab >= 1 && ldo >= gp.n_vocab && n_tiles == (gp.n_vocab + 15) / 16, WM_ERR_INVALID,
               "given_panel_close: %d ids in rows of %ld, %d tiles", gp.n_vocab, ldo, n_tiles);
    WM_REQUIRE(!mask || (long)mask_words * 32 >= gp.n_vocab, WM_ERR_INVALID, "given_panel_close: %d mask words do not cover %d ids",
               mask_words, gp.n_vocab);
    WM_REQUIRE(!gp.ts.rng || (gp.ts.key_ts && gp.ts.lse && gp.ts.ts_begin >= 0), WM_ERR_INVALID, "given_panel_close: incomplete timestamp-rule state");
    {
        WmProfScope ps(&ctx->prof, "given_panel_close", ctx->stream);
        given_panel_close_kernel<<<G, 512, 0, ctx->stream>>>(logits, ldo, gp.n_vocab, tilemax, n_tiles, w, n_prompt, gp, xd, mask, fallback_tok);
        WM_HIP(hipGetLastError());
    }
    return wm_given_panel_commit(ctx, gp, xd, stop, G, w, n_prompt, last);
}

// the second launch of wm_given_panel_close (which the product always makes through it; alone: the debug library's kernel tests)
int wm_given_panel_commit(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmXDev &xd, const WmStopDev &stop, int G, int w, int n_prompt,
                          bool last) {
    WM_TRY(panel_check(G, w, "given_panel_commit"));
    WM_REQUIRE(xd.logprob && gp.seq && gp.pos && gp.wtok && gp.wlp && (!gp.ts.rng || (gp.chist && gp.crng && gp.ts.hist)), WM_ERR_INVALID,
               "given_panel_commit: needs the extended decode and the round's state");
    WM_REQUIRE(!stop.done || (stop.live_rows && stop.n_live), WM_ERR_INVALID, "given_panel_commit: incomplete stop state");
    WmProfScope ps(&ctx->prof, "given_panel_commit", ctx->stream);
    given_panel_commit_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(gp, xd, stop, G, w, n_prompt, last ? 1 : 0);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
