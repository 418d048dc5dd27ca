// dtw.h -- the per-cell rule and the backtrace move of the dynamic time warping behind word-level timestamps (wm_align).
// Host and device: the DTW kernel of align.hip and the CPU restatement in tests/ (a host build of this header) run the same
// arithmetic.
//
// openai-whisper's dtw_cpu (whisper/timing.py), in f32.  cost[0][0] = 0, every other border cell +inf.  For cell (i, j)
// with c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]:
//     c0 < c1 && c0 < c2  -> (c0, 0);   else c1 < c0 && c1 < c2 -> (c1, 1);   else (c2, 2)
// cost[i][j] = x[i-1][j-1] + c (ONE f32 add), trace[i][j] = that code.  openai-whisper's CPU path runs the same rule in f64
// and its CUDA path runs f32 with another tie order; f32 with the CPU rule lets a numpy restatement reproduce the path bit
// for bit.  The backtrace starts at (N, M) with trace[0][:] = 2 and trace[:][0] = 1 and moves by wm_dtw_move.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WM_DTW_FN __host__ __device__ static inline
#else
#define WM_DTW_FN static inline
#endif

// cost of the cell, its trace code in *t
WM_DTW_FN float wm_dtw_cell(float x, float c0, float c1, float c2, int *t) {
    if (c0 < c1 && c0 < c2) { *t = 0; return x + c0; }
    if (c1 < c0 && c1 < c2) { *t = 1; return x + c1; }
    *t = 2;
    return x + c2;
}

// One backtrace step from (*i, *j) with trace code t (0: diagonal, 1: up, 2: left).  Leaving row i upwards means (i, j)
// is the first cell of row i on the path: text row i - 1 starts at audio frame j - 1 (openai-whisper's jump_times * 50).
// Returns that frame through *start_row / *start_frame (row -1: no row was left).
WM_DTW_FN void wm_dtw_move(int t, int *i, int *j, int *start_row, int *start_frame) {
    *start_row = -1;
    if (t == 0 || t == 1) {
        *start_row = *i - 1;
        *start_frame = *j - 1;
        *i -= 1;
    }
    if (t == 0 || t == 2) *j -= 1;
}
