// panel_rows.h -- device code shared by the two PANEL ROUNDS: a speculative round (spec.hip: stage, accept, commit) and a
// given-panel round (given_panel.hip: stage, close, commit).  Both step G windows x w positions at once -- row c * w + s of
// the panel step is window c at position pos + s -- keep a window's COMMITTED timestamp-rule state in a side area while the
// rules' range slots belong to the step's rows, stage a window's inputs with a replay of the rules along them, and close a
// row of the step by ONE wave with dec_close.h's calls.  Those pieces are stated ONCE here.  What the two rounds do NOT share
// stays in their files: the commit walks (spec: the group's lockstep cut; given: a stop per window) are different policies,
// and share only the state load and store (the callers, and the test that holds each piece).
#pragma once
#include "dec_close.h"

namespace {

// ------------------------------------------------------------------ a window's committed rule state ----------------------
// Window c's timestamp-rule history and ranges in ([..][4] ints each): the side area of a round, or the step path's own [G]
// slots (ts.hist, ts.rng).  The history is worked on as hs[4], which ts_advance advances in place.
__device__ __forceinline__ int4 panel_state_load(const int *hist, const int *rng, int c, int *hs) {
    const int4 h = *(const int4 *)(hist + c * 4);
    hs[0] = h.x; hs[1] = h.y; hs[2] = h.z; hs[3] = h.w;
    return *(const int4 *)(rng + c * 4);
}
__device__ __forceinline__ void panel_state_store(int *hist, int *rng, int c, const int *hs, int4 r) {
    *(int4 *)(hist + c * 4) = make_int4(hs[0], hs[1], hs[2], hs[3]);
    *(int4 *)(rng + c * 4) = r;
}

// ------------------------------------------------------------------ staging a window --------------------------------------
// Window c's inputs of a round of width w behind position pos: token tok_at(s, p) goes to position p = pos + s of the token
// buffer seq [..][G], s = 1 .. w - 1 (never at or past the context's end), and row (c, s) of the step gets the rules' ranges as
// they stand after the inputs up to its own, replayed from the window's committed state (hs, rng) into the rows' slots.  One
// thread per window; hs is left advanced.  tok_at returns a valid id (it indexes the embedding).
template <class TokAt>
__device__ __forceinline__ void panel_stage_window(const WmTsDev &ts, int *seq, int G, int c, int w, int pos, int n_ctx, int *hs, int4 rng,
                                                   TokAt tok_at) {
    if (ts.rng) *(int4 *)(ts.rng + (c * w) * 4) = rng;
    for (int s = 1; s < w; ++s) {
        const int p = pos + s;
        if (p >= n_ctx) break;
        const int tok = tok_at(s, p);
        seq[p * G + c] = tok;
        if (ts.rng) *(int4 *)(ts.rng + (c * w + s) * 4) = ts_advance(ts, hs, tok);
    }
}

// ------------------------------------------------------------------ the one-wave close of a panel row --------------------
// A row's close here is the arg-max close of dec_kernels.hip argmax_embed_body<true>: the same calls into dec_close.h
// (segments, totals, row_choose, row_logprob), by ONE wave per row, so winner, tie order, forced timestamps and log-prob are
// the plain step's.  It comes in two halves around a workgroup barrier that the CALLER places (its waves close different rows,
// some none): lane 0 writes the row's 16 segments, lanes 0 .. 15 read them -- the barrier argmax_embed_body has there.

// the row's best text key over its tiles, every lane holding it
__device__ __forceinline__ unsigned long long panel_row_key(const unsigned long long *row, int n_tiles, int lane) {
    unsigned long long key = 0ull;
    for (int t = lane; t < n_tiles; t += 64) {
        const unsigned long long k = row[t];
        key = k > key ? k : key;
    }
    return key_max_xor<64>(key);
}
// In front of the barrier: the key maximum of row b (returned) and its 16 segments into seg.
__device__ __forceinline__ unsigned long long panel_close_begin(const unsigned long long *tilemax, const WmXDev &xd, int b, int n_tiles,
                                                                int lane, float (*seg)[4]) {
    const long rb = (long)b * n_tiles;
    const unsigned long long key = panel_row_key(tilemax + rb, n_tiles, lane);
    lse_row_segments(xd, rb, n_tiles, false, 0, 1, lane, seg);
    return key;
}
// Behind the barrier: the row's total lt (every lane) and its decision.  seg == null: lt is the total a first call left and
// `key` a new maximum over keys rewritten since (given_panel.hip: the decision in front of the hand-over, the close behind it).
__device__ __forceinline__ RowChoice panel_close_choose(const WmTsDev &ts, int b, int n_tiles, int lane, unsigned long long key,
                                                        const float (*seg)[4], Lse &lt) {
    if (seg) {
        Lse la{-1e30f, 0.f};
        lt = Lse{-1e30f, 0.f};
        lse_row_total(seg, lane, lt, la);
    }
    return row_choose(ts, b, n_tiles, lane, key, lt.m);
}
// ... and what the wave's lane 0 stores for the row: the winner (the fallback where nothing is admissible) and its log-prob
// (lane 0 alone holds the log-prob: one load, made by the storing lane).
struct PanelRowClose {
    int tok;
    float lp;
};
__device__ __forceinline__ PanelRowClose panel_close_end(const WmTsDev &ts, const WmXDev &xd, int b, int n_tiles, int lane,
                                                         unsigned long long key, const float (*seg)[4], Lse &lt, int fallback_tok) {
    const RowChoice ch = panel_close_choose(ts, b, n_tiles, lane, key, seg, lt);
    PanelRowClose r{ch.key ? argmax_key_index(ch.key) : fallback_tok, 0.f};
    if (lane == 0) r.lp = row_logprob(ts, xd, b, n_tiles, ch, lt);
    return r;
}

}  // namespace
