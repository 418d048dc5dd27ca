// call_src.h -- what the host side of the transcribe, align, language-id and window-set calls share (transcribe.cpp,
// model_api.cpp): where a call's encoder input comes from, with its checks and stagers (call_src.cpp), and the small owners
// of streams' and events' lifetimes.  Internal: nothing here is part of the C ABI.
#pragma once
#include <stdlib.h>

#include <vector>

#include "model.h"

#define WM_MODEL(ctx)                                                               \
    WM_TRY(wm_ctx_make_current(ctx));                                               \
    WmModel *m = (ctx)->model;                                                      \
    WM_REQUIRE(m != nullptr, WM_ERR_STATE, "context was created without a model (use wm_create)")

inline bool wm_graphs_off() {   // every decode step is launched eagerly
    static const bool off = getenv("WM_NO_GRAPH") != nullptr;
    return off;
}

// Capture what `enqueue` launches on the stream into *out (whatever it held is destroyed first) and instantiate it.  A
// half-captured graph is of no use: on any failure *out is left empty; `what` names the graph in the error.
template <typename F>
int wm_capture_graph(hipStream_t stream, WmGraph *out, const char *what, F &&enqueue) {
    out->destroy();
    WM_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int crc = enqueue();
    const hipError_t ce = hipStreamEndCapture(stream, &out->g);
    if (crc != WM_OK || ce != hipSuccess) {
        if (ce != hipSuccess) out->g = nullptr;
        out->destroy();
        if (crc != WM_OK) return crc;
        WM_HIP(ce);
    }
    if (hipGraphInstantiate(&out->e, out->g, nullptr, nullptr, 0) != hipSuccess) {
        out->e = nullptr;
        out->destroy();
        wm_set_error("hipGraphInstantiate failed for %s", what);
        return WM_ERR_HIP;
    }
    return WM_OK;
}

// ---------------------------------------------------------------- owners ----
// Error paths: no asynchronous copy may outlive its host source.  Declared AFTER the buffers it fences (a member: last), so
// that the stream has drained when they die.
struct WmStreamFence {
    hipStream_t s = nullptr;
    bool on = true;
    ~WmStreamFence() { if (on && s) (void)hipStreamSynchronize(s); }
};

// N events, destroyed with the object
template <int N>
struct WmEvents {
    hipEvent_t e[N] = {};
    WmEvents() = default;
    WmEvents(const WmEvents &) = delete;
    WmEvents &operator=(const WmEvents &) = delete;
    ~WmEvents() {
        for (auto &x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create() {
        for (auto &x : e) WM_HIP(hipEventCreate(&x));
        return WM_OK;
    }
    int create_untimed() {   // markers the host polls: never read for a time
        for (auto &x : e) WM_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
        return WM_OK;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// sum[i] += the milliseconds between ev[i] and ev[i + 1], i < n_stages (an interval that cannot be read adds nothing).
// no_encoder: the call read a window set -- [0] is the gather and there is no encoder stage [1].
inline void wm_add_stage_ms(const hipEvent_t *ev, int n_stages, bool no_encoder, float *sum) {
    float ms;
    for (int i = 0; i < n_stages; ++i)
        if (!(no_encoder && i == 1) && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) sum[i] += ms;
}

// ---------------------------------------------------------------- a call's audio ----
// where a call's encoder input comes from: PCM chunks [.][480000], or (mel non-null) mel windows -- row b is frames
// seek[b] .. seek[b] + n_frames[b] - 1 of the [n_mels][mel_len[b]] block at mel + mel_base[b] --, or (windows) nothing
// to encode at all: row b is window rows[b] (rows null: b) of an encoded set, whose cross-attention K/V is copied
struct WmAudioSrc {
    const void *pcm = nullptr;
    wm_dtype pcm_dtype = WM_F32;
    const float *mel = nullptr;
    const int64_t *mel_base = nullptr;
    const int32_t *mel_len = nullptr, *seek = nullptr, *n_frames = nullptr;
    bool windows = false;   // the wm_*_windows calls: `set` is the source (null: an invalid call)
    const wm_windows *set = nullptr;
    const int32_t *rows = nullptr;
};

// row b of a mel source: its window lies inside its block (`who` prefixes the message; align bounds n_frames tighter itself)
int wm_check_window(const WmAudioSrc &a, int b, const char *who);
// the pointers of a window source: the five of a mel call, or the set
int wm_check_src_pointers(const WmAudioSrc &a);
// a set may be read by the context that made it and by every context that shares that one's weights
int wm_check_set_owner(const wm_ctx *ctx, const wm_windows *w);
// the B rows of a call that reads a set: every one a window of the set, made for this context's weights
int wm_check_set_rows(const wm_ctx *ctx, const WmAudioSrc &a, int B, const char *who);
// The stagers of rows [b0, b0 + Bg) on the lane c (call_src.cpp): the PCM in device memory; the encoder input; the
// cross-attention K/V in m->xkv.  `win` and `map` are the CALLER's: sources of asynchronous uploads.
int wm_stage_pcm(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void **d_pcm);
int wm_stage_mel(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void *d_pcm, std::vector<WmMelWin> &win,
                 const float **enc_mel, const WmMelWin **enc_win);
int wm_stage_cross_kv(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void *d_pcm, std::vector<WmMelWin> &win,
                      std::vector<int32_t> &map, hipEvent_t staged);
