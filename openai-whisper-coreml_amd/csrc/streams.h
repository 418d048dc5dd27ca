// streams.h -- a set of live audio streams (include/whisper_mi355x.h wm_streams): the object, its frame arithmetic as pure
// host functions, and the launchers of streams.hip.  The entries are in streams.cpp; the stage-1 launch is the stream rule
// of frontend.hip's f32 kernel.
#pragma once
#include "wm_internal.h"

constexpr int WM_STREAM_MIN_CAPACITY = 3003;   // a full 3000-frame window plus the provisional frames
constexpr int WM_STREAM_MAX_WINDOW = 3000;
constexpr int WM_STREAM_FPB = 64;              // frames per workgroup of the stage-1 kernel

// Frame t reads the samples [160 t - 200, 160 t + 200); an index n < 0 reads sample -n, so frame 0 needs sample 200.
// final: frames whose every sample has arrived (a prefix); avail: frames that read at least one arrived sample.
inline int64_t wm_stream_final(int64_t n) { return n < 201 ? 0 : (n - 200) / WM_HOP + 1; }
inline int64_t wm_stream_avail(int64_t n) { return n <= 0 ? 0 : (n + 199) / WM_HOP + 1; }
// first sample that a frame which is not final still reads: where the carry begins
inline int64_t wm_stream_carry_start(int64_t n) {
    const int64_t f = wm_stream_final(n);
    return f * WM_HOP < 200 ? 0 : f * WM_HOP - 200;   // (frame 1 reads the reflected samples 1 .. 40: from sample 0)
}

struct wm_streams {
    int device = 0, S = 0, n_mels = 0, cap = 0;
    float *ring = nullptr;    // [S][n_mels][cap] raw log10(max(mel, 1e-10)), frame t in column t % cap
    float *fmax = nullptr;    // [S][cap] each frame's maximum over its mel rows
    float *carry = nullptr;   // [S][WM_STREAM_CARRY] staged f32 samples from wm_stream_carry_start(n) on
    std::vector<int64_t> n;        // samples received
    std::vector<int64_t> floor;    // first frame the ring can hold (0; wmdbg_streams_set_position: the first frame after it)
    std::vector<uint8_t> reflect;  // the stream began at sample 0
    std::vector<uint8_t> stale;    // provisional frames not computed yet (after wmdbg_streams_set_position)
    void *tab = nullptr;      // tables of a call
    size_t tab_bytes = 0;
    void *stage = nullptr;    // staging of a WM_MEM_HOST call's samples, row tables and output
    size_t stage_bytes = 0;
};

extern int g_wm_stream_min_capacity;   // streams.cpp; lowered by the debug library alone

// rows of a window call (streams.hip): block r = [n_mels][n] at out + out_base
struct WmStreamWin {
    long long out_base;
    int stream, col0, n, pad;
};
// carry[s] = samples [shift, shift + new_len) of [carry[s] | new samples of s], for every stream with n_new > 0
int wm_streams_carry_run(hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype, const WmStreamRec *d_rec, float *d_carry, int S);
int wm_streams_window_run(WmProfiler *prof, hipStream_t stream, const float *d_ring, const float *d_fmax, int n_mels, int cap,
                          const WmStreamWin *d_rows, int R, int max_n, float *d_out);
