// row_list.h -- the descending-key list of a row's admissible ids, stated ONCE: beam_topk_kernel (beam.hip) and
// alternatives_kernel (alternatives.hip) both call row_list_scan, so an alternatives list of n entries is the list of a beam
// of width n - 1 bit for bit.  One 16-wave workgroup (1024 threads) per row; a thread's ids are tid + 1024 i.
#pragma once
#include "stored_row.h"

// A thread's best admissible key below `bound`.  visit(n, v) sees every admissible id of the thread, ascending, with its
// stored value: the pass that a caller's own per-id sums share with the scan (stored_row.h row_for_each_admitted).
template <class Visit>
__device__ __forceinline__ unsigned long long row_list_local_best(const float *__restrict__ row, const RowAdmit &a,
                                                                  unsigned long long bound, Visit visit) {
    unsigned long long best = 0ull;
    row_for_each_admitted(row, a, [&](int n, float v) {
        visit(n, v);
        const unsigned long long k = argmax_key(v, n);
        if (k < bound && k > best) best = k;
    });
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
