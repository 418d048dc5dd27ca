// stored_row.h -- device code shared by the kernels that run on a decode row BETWEEN the logits launch (which stored the f32
// row, penalised and biased, and left the per-tile partials) and the close: beam_topk_kernel (beam.hip), sample_trunc_kernel
// (sample_trunc.hip), alternatives_kernel (alternatives.hip), given_tokens_kernel (given.hip) -- one 16-wave workgroup (1024
// threads) per row -- and the one-wave close of given_panel.hip.  Stated ONCE here: the admissible set of a row and its one-id
// test, the unrolled pass over a row's admissible ids, the prologue that takes `forced` and the normaliser from the partials,
// and the hand-over that leaves one id in the row's keys.  Each is order-sensitive; the next row feature calls these and
// copies none (the callers, and the test that holds each piece).
#pragma once
#include "dec_close.h"

namespace {

// The admissible set of a row: the allowed text range (none when the sum rule forced a timestamp) and the allowed timestamp
// range, less the suppress bitmap and the row's ban bitmap (no-repeat n-grams, sequence-bias bans); either bitmap may be null.
struct RowAdmit {
    int V;
    int4 rng;
    bool forced;
    const unsigned *mrow, *brow;
};

// The admissible set of row b at position pos.  mask (nullable): the suppress bitmap, whose row for the FIRST generated position
// lies mask_words behind the every-position row (a caller that never sees that position passes mask_words 0); ban (nullable):
// the rows' ban bitmaps [rows][ban_words] -- repetition rules, sequence bias, constraint (the penalty is already in the stored
// logits); forced: the row's sum rule (stored_row_prologue, row_choose).
__device__ __forceinline__ RowAdmit row_admit_set(int V, const WmTsDev &ts, const unsigned *mask, int mask_words, const unsigned *ban,
                                                  int ban_words, int b, int pos, int n_prompt, bool forced) {
    RowAdmit a;
    a.V = V;
    a.rng = make_int4(0, V, 0, 0);
    if (ts.rng) a.rng = *(const int4 *)(ts.rng + b * 4);
    a.forced = forced;
    a.mrow = mask ? mask + (pos == n_prompt - 1 ? mask_words : 0) : nullptr;
    a.brow = ban ? ban + (long)b * ban_words : nullptr;
    return a;
}

// the ranges alone: is n an allowed text id or an allowed timestamp?  (For a caller that holds the bitmap words already.)
__device__ __forceinline__ bool row_in_ranges(const RowAdmit &a, int n) {
    const bool in_text = !a.forced && n >= a.rng.x && n < a.rng.y, in_ts = n >= a.rng.z && n < a.rng.w;
    return in_text || in_ts;
}
// The test for ONE id (the per-id test of row_for_each_admitted below): is n in the row's admissible set?  The bitmap words of
// n are read whatever n is: the caller keeps an id outside [0, V) away.
__device__ __forceinline__ bool row_admits(const RowAdmit &a, int n) {
    const unsigned w = (a.mrow ? a.mrow[n >> 5] : 0u) | (a.brow ? a.brow[n >> 5] : 0u);
    return n >= 0 && n < a.V && row_in_ranges(a, n) && !((w >> (n & 31)) & 1u);
}

// One thread's pass over a row in a 1024-thread workgroup: f(n, v) for every admissible id n = tid + 1024 i of the thread,
// ascending, with its stored value (-inf and NaN included: the caller filters).
// A pass is latency-bound (one workgroup, ~51 ids per thread from L2): the loads of ROW_PASS_UNROLL ids -- value, suppress word,
// ban word, none depending on another -- are requested together, then tested in ascending order.
constexpr int ROW_PASS_UNROLL = 8;
template <class F>
__device__ __forceinline__ void row_for_each_admitted(const float *__restrict__ row, const RowAdmit &a, F f) {
    for (int n0 = threadIdx.x; n0 < a.V; n0 += 1024 * ROW_PASS_UNROLL) {
        float v[ROW_PASS_UNROLL];
        unsigned w[ROW_PASS_UNROLL];
#pragma unroll
        for (int j = 0; j < ROW_PASS_UNROLL; ++j) {
            const int n = n0 + j * 1024, nc = n < a.V ? n : a.V - 1;   // (clamped: the test below drops it)
            v[j] = row[nc];
            w[j] = (a.mrow ? a.mrow[nc >> 5] : 0u) | (a.brow ? a.brow[nc >> 5] : 0u);
        }
#pragma unroll
        for (int j = 0; j < ROW_PASS_UNROLL; ++j) {
            const int n = n0 + j * 1024;
            if (n >= a.V || !row_in_ranges(a, n) || ((w[j] >> (n & 31)) & 1u)) continue;
            f(n, v[j]);
        }
    }
}

// The prologue of a 16-wave stored-row kernel: the row's decision between text and timestamps, from the partials.  The log-sum-exp
// of the allowed text in dec_close.h's fixed orders (16 segments, wave 0's total; `sot`: the unfiltered one beside it), the best
// allowed text key over the row's tiles -- read only under the timestamp rules: row_choose asks whether there is one, and looks
// at no key without them -- then wave 0's row_choose and finish(ch, lt, la), every lane of wave 0 holding the arguments: the
// kernel's lane 0 writes what that kernel keeps (`forced`, the normaliser, the best value) to its own shared words, which every
// thread may read behind the call.
// The function contains two workgroup barriers: EVERY thread of the workgroup calls it, so a kernel's early returns stand in
// front of it and are workgroup-uniform.  Every read of the row's keys lies in front of the second barrier: a rewrite of them
// (row_hand_over) may begin behind the call.  seg_s: [16][4] floats, red_s: [16] words of the workgroup.
template <class Finish>
__device__ __forceinline__ void stored_row_prologue(const WmTsDev &ts, const WmXDev &xd, const unsigned long long *tilemax, int b,
                                                    int n_tiles, bool sot, float (*seg_s)[4], unsigned long long *red_s, Finish finish) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rb = (long)b * n_tiles;
    lse_row_segments(xd, rb, n_tiles, sot, wave, 16, lane, seg_s);
    {   // the best allowed text key of the row (decides the sum rule with the timestamps' log-sum-exp)
        unsigned long long key = 0ull;
        if (ts.rng) {
            for (int t = threadIdx.x; t < n_tiles; t += 1024) {
                const unsigned long long k = tilemax[rb + t];
                key = k > key ? k : key;
            }
            key = key_max_xor<64>(key);
        }
        if (lane == 0) red_s[wave] = key;
    }
    __syncthreads();
    if (wave == 0) {
        Lse lt{-1e30f, 0.f}, la{-1e30f, 0.f};
        lse_row_total(seg_s, lane, lt, la);
        unsigned long long key = lane < 16 ? red_s[lane] : 0ull;
        key = __shfl(key_max_xor<16>(key), 0);
        finish(row_choose(ts, b, n_tiles, lane, key, lt.m), lt, la);
    }
    __syncthreads();
}
// the best value of the row's admissible set, as the prologue's finish sees it (at or below -1e30: nothing is admissible)
__device__ __forceinline__ float row_best_value(const RowChoice &ch, Lse lt) {
    return ch.forced ? ch.lts.m : fmaxf(lt.m, ch.lts.m);   // (lts: (-1e30, 0) without timestamp rules)
}

// The hand-over: only the id of `win` = argmax_key(value, id) is left in row rb / n_tiles' per-tile keys, and the caller stores
// the value at xd.win[row_win_slot(..)].  The log-sum-exp partials stay, so argmax_embed_body and dec_close.h run unchanged on
// the row and the log-prob is value - the row's own normaliser.  A timestamp handed over where the sum rule did not force one
// leaves the smallest key in the text keys (tile 0), so that row_choose still sees admissible text below it (its decision reads
// lt.m).  The cases, through row_choose / row_logprob of the close (K = win > 1; F = the row's `forced`):
//   text, not F           : tilemax = {K}, key_ts = {}        -> kts 0: not forced, key K, norm over text + timestamps
//   text, F               : the same keys.  Not admissible: value -inf, the close's norm is the finite one over text + timestamps
//                           instead of the timestamps' (row_choose cannot force a timestamp and keep a text id) -- -inf either way
//   timestamp, not F      : tilemax = {1 in tile 0}, key_ts = {K} -> key 1: text_best = lt.m, lse <= lt.m as before: not forced,
//                           the winner is max(K, 1) = K, norm over text + timestamps
//   timestamp, F          : tilemax = {}, key_ts = {K}        -> key 0: forced, key K, norm over the timestamps
//   timestamp rules off   : tilemax = {K}                     -> key K, norm over the allowed ids
// and an id that is not admissible differs from an admissible one in its value alone.
// Thread tid of `stride` threads (a 1024-thread workgroup, or the 64 lanes of a row's wave) rewrites tiles tid, tid + stride, ...;
// every read of the row's keys by those threads must be behind a barrier or consumed.
__device__ __forceinline__ void row_hand_over(const WmTsDev &ts, unsigned long long *tilemax, long rb, int n_tiles, bool forced,
                                              unsigned long long win, int tid, int stride) {
    const int tok = argmax_key_index(win), wt = tok >> 4;
    const int side = (ts.rng && tok >= ts.ts_begin) ? 1 : 0;
    const int t_first = ts.ts_begin >> 4;
    for (int t = tid; t < n_tiles; t += stride) {
        tilemax[rb + t] = (side == 0 && t == wt) ? win : ((side == 1 && !forced && t == 0) ? 1ull : 0ull);
        if (ts.rng && t >= t_first) ts.key_ts[rb + t] = (side == 1 && t == wt) ? win : 0ull;
    }
}

}  // namespace
