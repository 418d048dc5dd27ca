// row_list.h -- the descending-key list of a row's admissible ids, stated ONCE: beam_topk_kernel (beam.hip) and
// alternatives_kernel (alternatives.hip) both call row_list_scan, so an alternatives list of n entries is the list of a beam
// of width n - 1 bit for bit.  One 16-wave workgroup (1024 threads) per row; a thread's ids are tid + 1024 i.
#pragma once
#include "dec_close.h"

// The admissible set of a row: the allowed text range (none when the sum rule forced a timestamp) and the allowed timestamp
// range, less the suppress bitmap and the row's ban bitmap (no-repeat n-grams, sequence-bias bans); either bitmap may be null.
struct RowAdmit {
    int V;
    int4 rng;
    bool forced;
    const unsigned *mrow, *brow;
};

// The same test for ONE id (the per-id test of row_list_local_best below): is n in the row's admissible set?
__device__ __forceinline__ bool row_admits(const RowAdmit &a, int n) {
    const bool in_text = !a.forced && n >= a.rng.x && n < a.rng.y, in_ts = n >= a.rng.z && n < a.rng.w;
    const unsigned w = (a.mrow ? a.mrow[n >> 5] : 0u) | (a.brow ? a.brow[n >> 5] : 0u);
    return n >= 0 && n < a.V && (in_text || in_ts) && !((w >> (n & 31)) & 1u);
}

// A thread's best admissible key below `bound`.  visit(n, v) sees every admissible id of the thread, ascending, with its
// stored value: the pass that a caller's own per-id sums share with the scan.
// A pass is latency-bound (one workgroup, ~51 ids per thread from L2): the loads of ROW_LIST_UNROLL ids -- value, suppress word,
// ban word, none depending on another -- are requested together, then tested in ascending order (sample_trunc.hip's st_for_each).
constexpr int ROW_LIST_UNROLL = 8;
template <class Visit>
__device__ __forceinline__ unsigned long long row_list_local_best(const float *__restrict__ row, const RowAdmit &a,
                                                                  unsigned long long bound, Visit visit) {
    unsigned long long best = 0ull;
    for (int n0 = threadIdx.x; n0 < a.V; n0 += 1024 * ROW_LIST_UNROLL) {
        float v[ROW_LIST_UNROLL];
        unsigned w[ROW_LIST_UNROLL];
#pragma unroll
        for (int j = 0; j < ROW_LIST_UNROLL; ++j) {
            const int n = n0 + j * 1024, nc = n < a.V ? n : a.V - 1;   // (clamped: the test below drops it)
            v[j] = row[nc];
            w[j] = (a.mrow ? a.mrow[nc >> 5] : 0u) | (a.brow ? a.brow[nc >> 5] : 0u);
        }
#pragma unroll
        for (int j = 0; j < ROW_LIST_UNROLL; ++j) {
            const int n = n0 + j * 1024;
            const bool in_text = !a.forced && n >= a.rng.x && n < a.rng.y, in_ts = n >= a.rng.z && n < a.rng.w;
            if (n >= a.V || !(in_text || in_ts) || ((w[j] >> (n & 31)) & 1u)) continue;
            visit(n, v[j]);
            const unsigned long long k = argmax_key(v[j], n);
            if (k < bound && k > best) best = k;
        }
    }
    return best;
}

// The K best admissible ids of the row in descending argmax_key order (higher value first, equal values lower id first), with
// log-probs value - norm.  Every thread scans once (visit sees that pass); then K rounds of a workgroup-wide maximum, and only
// a round's winner rescans below the key it retires.  -inf (and NaN) is never listed.  Thread 0 calls emit(r, key, lp) for
// entry r; every thread gets the count.  red_s: [2][16] words of the workgroup.  The reductions are maxima: any order, same bits.
template <class Visit, class Emit>
__device__ __forceinline__ int row_list_scan(const float *__restrict__ row, const RowAdmit &a, int K, float norm,
                                             unsigned long long (*red_s)[16], Visit visit, Emit emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long mine = row_list_local_best(row, a, ~0ull, visit);
    int count = 0;
    for (int r = 0; r < K; ++r) {   // K rounds of a workgroup-wide maximum; the winner's thread retires it
        unsigned long long key = key_max_xor<64>(mine);
        if (lane == 0) red_s[(r + 1) & 1][wave] = key;
        __syncthreads();
        key = lane < 16 ? red_s[(r + 1) & 1][lane] : 0ull;
        key = __shfl(key_max_xor<16>(key), 0);
        if (key == 0ull) break;                       // nothing admissible is left (uniform)
        const float lp = argmax_key_value(key) - norm;
        if (!(lp > -INFINITY)) break;                 // -inf (and NaN) is never listed (uniform)
        if (threadIdx.x == 0) emit(r, key, lp);
        ++count;
        if (mine == key) mine = row_list_local_best(row, a, key, [](int, float) {});
    }
    return count;
}
