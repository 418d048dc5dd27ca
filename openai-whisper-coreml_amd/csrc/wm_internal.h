// wm_internal.h -- private declarations shared by the translation units of
// libwhisper_mi355x.so (gfx950 only; nothing here is part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/whisper_mi355x.h"

// ---------------------------------------------------------------- error plumbing -----
void wm_set_error(const char *fmt, ...);

#define WM_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            wm_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr,               \
                         hipGetErrorString(_e));                                          \
            return WM_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)

#define WM_TRY(expr)                                                                      \
    do {                                                                                  \
        int _s = (expr);                                                                  \
        if (_s != WM_OK) return _s;                                                       \
    } while (0)

#define WM_REQUIRE(cond, code, ...)                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            wm_set_error(__VA_ARGS__);                                                    \
            return (code);                                                                \
        }                                                                                 \
    } while (0)

// Every int-returning entry point of the C ABI is a function-try-block closed by this: no C++ exception (bad_alloc /
// length_error from a std::vector sized by caller- or file-supplied numbers, ...) ever crosses the FFI.
#define WM_API_CATCH                                                                      \
    catch (const std::bad_alloc &) {                                                      \
        wm_set_error("out of host memory");                                               \
        return WM_ERR_NOMEM;                                                              \
    }                                                                                     \
    catch (const std::exception &e) {                                                     \
        wm_set_error("internal error: %s", e.what());                                     \
        return WM_ERR_NOMEM;                                                              \
    }                                                                                     \
    catch (...) {                                                                         \
        wm_set_error("internal error (unknown exception)");                               \
        return WM_ERR_NOMEM;                                                              \
    }

// ---------------------------------------------------------------- fixed geometry -----
// Literals of the reference front end (stft/src/lib.rs:24,26,35-37,50-52,112,116).
constexpr int WM_N_SAMPLES = 480000;  // 16000 * 30
constexpr int WM_N_FFT = 400;
constexpr int WM_HOP = 160;
constexpr int WM_N_BINS = 201;
constexpr int WM_N_FRAMES = 3000;
constexpr int WM_MEL_MAXW = 32;  // widest supported filter band (80 mels: 14)

typedef unsigned short bf16_t;  // raw bf16 bits in HBM

// ---------------------------------------------------------------- profiling ----------
struct WmProfFamily {
    double ms = 0.0;
    long n = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct WmProfiler {
    bool on = false;
    std::map<std::string, WmProfFamily> fam;
    std::vector<hipEvent_t> pool;
    hipEvent_t get();
    void begin(const char *name, hipStream_t s, hipEvent_t *e0);
    void end(const char *name, hipStream_t s, hipEvent_t e0);
    void drain();
    void reset();
    ~WmProfiler();
};

struct WmProfScope {
    WmProfiler *p;
    const char *name;
    hipStream_t s;
    hipEvent_t e0 = nullptr;
    WmProfScope(WmProfiler *p_, const char *n, hipStream_t s_) : p(p_), name(n), s(s_) {
        if (p && p->on) p->begin(name, s, &e0);
    }
    ~WmProfScope() {
        if (p && p->on && e0) p->end(name, s, e0);
    }
};

// ---------------------------------------------------------------- front end ----------
struct WmFrontend {
    // DFT-as-MFMA tables: rows n = 1..200, 208 columns (bins 0..200, rest zero).
    float *cos32 = nullptr, *sin32 = nullptr, *win32 = nullptr;
    double *cos64 = nullptr, *sin64 = nullptr, *win64 = nullptr;
    // banded mel filters per supported n_mels (index 0: 80, index 1: 128)
    int *band_start[2] = {nullptr, nullptr};
    int *band_len[2] = {nullptr, nullptr};
    float *band_w[2] = {nullptr, nullptr};  // [n_mels][WM_MEL_MAXW]
    int band_maxw[2] = {0, 0};              // widest band of the filterbank (the LDS-resident copy of the f32 kernel holds 16)
    void *gmax = nullptr;                   // per-chunk encoded maxima (u64 per chunk)
    int gmax_cap = 0;
    void *scratch = nullptr;                // staging for host-pointer calls
    size_t scratch_bytes = 0;
    void *long_tab = nullptr;               // wm_logmel_long: recording and workgroup tables (WmLongRec, int2)
    size_t long_tab_bytes = 0;
    bool ready = false;
};

// wm_logmel_long's geometry (frontend.hip): one record per recording, one (recording, first frame) pair per workgroup
struct WmLongRec {
    long long base;  // first sample of the recording in pcm
    long long out;   // element offset of its [n_mels][T] block in the output
    int len;         // samples (>= 0)
    int T;           // frames: (len + 480000) / 160
};
struct WmLongTab {
    const WmLongRec *rec;
    const int2 *blk;
};

// wm_streams_push's geometry (frontend.hip, streams.hip): one record per stream of the set, one (stream, first span sample
// relative to the carry, ring column of the first frame, frames) entry per workgroup of up to 64 frames.  Everything a
// kernel sees is relative to the carry's first sample or to the ring: absolute stream time stays on the host, in 64 bits.
constexpr int WM_STREAM_CARRY = 400;   // samples of a stream that frames which are not final still need: at most 399
struct WmStreamRec {
    long long pcm_base;  // first new sample of the stream in pcm
    int carry_len;       // staged f32 samples held from earlier pushes (<= 399)
    int n_new;           // new samples (0: the stream is not part of this push)
    int reflect;         // the stream began at its sample 0: indices below it are reflected (else they read 0)
    int shift;           // the next carry begins at this index of [carry | new samples]
    int new_len;         // ... and holds this many samples (<= 399)
    int pad;
};
struct WmStreamTab {
    const WmStreamRec *rec;
    const int4 *blk;
    const float *carry;  // [S][WM_STREAM_CARRY]
    float *fmax;         // [S][cap] a frame's maximum over its mel rows, by ring column
    int cap;             // ring columns per stream
};

int wm_frontend_init(WmFrontend *fe, hipStream_t stream);
// One launch of the f32 stage-1 kernel under the stream rule: n_blk workgroups of tab.blk, raw log10 values into
// d_ring [S][n_mels][tab.cap], per-frame maxima into tab.fmax.
int wm_frontend_run_stream(WmFrontend *fe, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype, int n_mels,
                           const WmStreamTab &tab, int n_blk, float *d_ring);
void wm_frontend_destroy(WmFrontend *fe);
// Device-pointer core: pcm [n][480000] (dtype) -> out [n][n_mels][3000] (f32 or f64).
int wm_frontend_run(WmFrontend *fe, WmProfiler *prof, hipStream_t stream, const void *d_pcm,
                    wm_dtype pcm_dtype, int n_chunks, int n_mels, void *d_out,
                    wm_dtype out_dtype);
// openai-whisper log_mel_spectrogram(audio, padding=480000), f32, of R recordings back to back in d_pcm: recording r =
// d_pcm[offs[r] .. offs[r + 1]) (offs: host) -> d_out, recording r's [n_mels][(len_r + 480000) / 160] after the previous ones.
int wm_frontend_run_long(WmFrontend *fe, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype,
                         const int64_t *offs, int R, int n_mels, float *d_out);
// frames of a recording of len samples in that layout
inline int64_t wm_long_frames(int64_t len) { return (len + WM_N_SAMPLES) / WM_HOP; }
// Host-side slaney mel filterbank generator (librosa.filters.mel semantics; used for
// n_mels = 128 and validated against the reference's m80.npy at n_mels = 80).
void wm_mel_filterbank(int n_mels, std::vector<float> &out /* [n_mels][201] */);
const float *wm_mel80_table();

// ---------------------------------------------------------------- resampler (resample.hip) ----------
constexpr int WM_RS_TARGET_RATE = 16000;
constexpr int WM_RS_MIN_RATE = 4000, WM_RS_MAX_RATE = 192000;
constexpr int WM_RS_MAX_L = 640;        // 16000 / gcd(rate, 16000): 11025 Hz and its multiples are the largest
constexpr int WM_RS_MAX_CHANNELS = 8;
struct WmRsFilter {
    int L = 0, M = 0, K = 0, T4 = 0;    // T4: taps per output, rounded up to a multiple of 4
    float *d_tab = nullptr;             // phase table [L][T4] on the device
};
struct WmResampler {
    std::map<int, WmRsFilter> filt;     // by input rate, built and uploaded on first use
    void *tab = nullptr;                // recording and workgroup tables of a call
    size_t tab_bytes = 0;
};
bool wm_resample_params(long long sample_rate, int *L, int *M, int *K);   // false: unsupported rate
void wm_resample_prototype(int L, int M, int K, std::vector<float> &h);   // h[0 .. 2K], f64 rounded once to f32
void wm_resample_destroy(WmResampler *rs);
// Device-pointer core of wm_resample_16k: recording r = d_pcm[offs[r] .. offs[r + 1]) (interleaved, n_channels[r] channels,
// sample_rates[r] Hz) -> d_out, its ceil(n L / M) samples after those of the recordings before it.  One launch.
int wm_resample_run(WmResampler *rs, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype,
                    const int64_t *offs, const int32_t *n_channels, const int32_t *sample_rates, int R, float *d_out);
// Device-pointer core of wm_resample_16k_mix: the same with n_rows[r] output signals per recording, signal (r, o) under the
// weights mix[row (r, o)] (n_rows, mix: host; the rows back to back) -> d_out, the signals in (r, o) order.  One launch.
int wm_resample_mix_run(WmResampler *rs, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype,
                        const int64_t *offs, const int32_t *n_channels, const int32_t *sample_rates, int R, const int32_t *n_rows,
                        const float *mix, float *d_out);

// ---------------------------------------------------------------- per-channel activity (channel_activity.hip) ----------
constexpr int WM_CHANACT_TILE = 64;     // frames per workgroup
struct WmChanAct {
    void *tab = nullptr;                // signal and workgroup tables of a call
    size_t tab_bytes = 0;
};
void wm_chanact_destroy(WmChanAct *ca);
// Device-pointer core of wm_channel_activity: signal s = d_pcm[offs[s] .. offs[s + 1]) (offs: host) -> d_act, its
// ceil(N_s / WM_ACTIVITY_HOP) values after those of the signals before it.  One launch.
int wm_chanact_run(WmChanAct *ca, WmProfiler *prof, hipStream_t stream, const float *d_pcm, const int64_t *offs, int S, float *d_act);

// ---------------------------------------------------------------- speech-activity energy (vad.hip) ----------
constexpr int WM_VAD_MAX_SMOOTH = 31;
struct WmVad {
    void *tab = nullptr;                // recording and workgroup tables of a call
    size_t tab_bytes = 0;
};
void wm_vad_destroy(WmVad *vad);
// Device-pointer core of wm_vad_energy: recording r's band is the n_band rows of stride[r] frames from element row0[r] of
// d_mel (row0, stride, n_frames: host) -> d_raw (nullable) and d_energy, n_frames[r] values after those of the recordings
// before it.  One launch.
int wm_vad_run(WmVad *vad, WmProfiler *prof, hipStream_t stream, const float *d_mel, const int64_t *row0, const int32_t *stride,
               const int32_t *n_frames, int R, int n_band, int smooth, float *d_raw, float *d_energy);

// ---------------------------------------------------------------- context ------------
struct WmModel;  // model.h
struct wm_ctx;

// Model-call overrides a DEBUG build can install on a context (libwhisper_mi355x_dbg.so: wmdbg_set_precision -> the
// all-fp32 path of f32_path.hip).  The product library has no code that sets them: always null there.
struct WmDebugHooks {
    int (*encode_dev)(wm_ctx *ctx, const float *d_mel, int B, float *d_xa);
    int (*decode_logits_dev)(wm_ctx *ctx, const int32_t *host_tokens /*[B][T]*/, int B, int T, const float *d_xa,
                             float *d_logits /*[B][T][n_vocab]*/);
};

struct wm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    WmProfiler prof;
    WmFrontend fe;
    WmResampler rs;
    WmVad vad;
    WmChanAct chanact;
    WmModel *model = nullptr;
    float stage_ms[3] = {0, 0, 0};
    std::vector<wm_ctx *> lanes;  // weight-sharing clones owned by this context (wm_transcribe_greedy)
    const WmDebugHooks *dbg_hooks = nullptr;
    int max_lanes = 0;            // wm_set_lanes: decode groups in flight per wm_transcribe_greedy call (0: $WM_LANES, default 3)
    // SUB-CHIP LANES (round 6).  A context whose stream was created with a CU mask (hipExtStreamCreateWithCUMask) runs
    // everything it launches on `n_cus` of the 256 CUs: the CUs [cu_lo, cu_hi) of every XCD.  Two or
    // three SMALL decode groups (latency-bound launch chains) then run side by side on disjoint CUs instead of flooding
    // all 256 CUs with every launch and serialising at the CU level (tx_plan.cpp, the group policy).
    int n_cus = 256, cu_lo = 0, cu_hi = 32;   // the CUs [cu_lo, cu_hi) of every XCD
    std::vector<wm_ctx *> part_lanes[2];   // [0]: the two clones of the 2-way partition, [1]: the three of the 3-way one (created on first use)
    bool no_cu_masks = false;              // a CU-masked stream could not be created on this device: the policy stays unmasked
    std::map<int, wm_ctx *> solo_lanes;    // probes (debug knob lane_solo_cus): a clone confined to the first n CUs of every XCD
};
// fn(c) -> status for the context itself (with_self) and every lane it owns; the first status that is not WM_OK ends the
// walk and is returned
template <typename F>
int wm_for_each_lane(wm_ctx *ctx, bool with_self, F &&fn) {
    if (with_self) WM_TRY(fn(ctx));
    for (wm_ctx *lane : ctx->lanes) WM_TRY(fn(lane));
    for (auto &v : ctx->part_lanes)
        for (wm_ctx *lane : v) WM_TRY(fn(lane));
    for (auto &kv : ctx->solo_lanes) WM_TRY(fn(kv.second));
    return WM_OK;
}
// weight-sharing clone of `parent` whose stream is confined to the CUs [cu_lo, cu_hi) of every XCD (api.cpp)
int wm_clone_cus(wm_ctx *parent, int cu_lo, int cu_hi, wm_ctx **out);
// CU mask (256 bits) of the CUs [cu_lo, cu_hi) of every XCD; returns the CU count
int wm_cu_mask(int cu_lo, int cu_hi, uint32_t mask[8]);

int wm_ctx_make_current(const wm_ctx *ctx);
double wm_rank_score(double sum, int n_text, float length_penalty);   // api.cpp: the MaximumLikelihoodRanker's score
// (decode groups, lanes and a group's tables of a transcribe call: tx_plan.h)

// ---------------------------------------------------------------- launch-shape experiment knobs
// Launch shapes are chosen by fixed rules (dec_launch.cpp: the decode plans; gemm.hip wm_gemm): the
// product library reads NO environment variable for them, so nothing outside the process's own calls can change a launch
// shape in a library whose contract is bit-level batch invariance.  The A/B probes of tools/ change these fields through
// wmdbg_set_tuning(), which exists in libwhisper_mi355x_dbg.so only (debug_hooks.cpp).  A value of 0 / the default below
// means "the product's rule".
#include "wm_tuning.h"   // struct WmTuning
extern WmTuning g_wm_tuning;   // api.cpp

// wm_transcribe_greedy calls in flight per device (any context, any host thread): a decode group that shares the chip
// with others launches its cross-attention as short-lived workgroups (model.h WmDecodeMode::xattn_shared).
#include <atomic>
extern std::atomic<int> g_wm_active_decodes[64];   // api.cpp
