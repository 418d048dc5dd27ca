// api.cpp -- the C ABI of libwhisper_mi355x.so (declared in include/whisper_mi355x.h):
// context life cycle, error reporting, the front-end entry points (boundary #1), device
// memory helpers and the HIP-event profiler.  The model entry points (boundary #2) are in
// model_api.cpp and transcribe.cpp.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "wm_internal.h"
#include "model.h"

WmTuning g_wm_tuning;   // wm_internal.h: defaults = the product; only the debug library has a setter
std::atomic<int> g_wm_active_decodes[64];

// ---------------------------------------------------------------- errors -------------
static thread_local std::string g_last_error;

void wm_set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

extern "C" const char *wm_last_error(void) { return g_last_error.c_str(); }

// ---------------------------------------------------------------- profiler -----------
hipEvent_t WmProfiler::get() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void WmProfiler::begin(const char *, hipStream_t s, hipEvent_t *e0) {
    *e0 = get();
    (void)hipEventRecord(*e0, s);
}
void WmProfiler::end(const char *name, hipStream_t s, hipEvent_t e0) {
    hipEvent_t e1 = get();
    (void)hipEventRecord(e1, s);
    WmProfFamily &f = fam[name];
    f.pending.emplace_back(e0, e1);
    if (f.pending.size() >= 4096) drain();
}
void WmProfiler::drain() {
    for (auto &kv : fam) {
        for (auto &pr : kv.second.pending) {
            (void)hipEventSynchronize(pr.second);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                kv.second.ms += ms;
                kv.second.n += 1;
            }
            pool.push_back(pr.first);
            pool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}
void WmProfiler::reset() {
    drain();
    fam.clear();
}
WmProfiler::~WmProfiler() {
    for (auto &kv : fam)
        for (auto &pr : kv.second.pending) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
}

// ---------------------------------------------------------------- context ------------
int wm_ctx_make_current(const wm_ctx *ctx) {
    WM_REQUIRE(ctx != nullptr, WM_ERR_INVALID, "null context");
    WM_HIP(hipSetDevice(ctx->device));
    return WM_OK;
}

// Bit i of a CU mask enables CU i / 8 of XCD i % 8 (the KFD deals the bits round-robin over the 8 XCCs; measured with the
// census of tools/cu_mask_lab.hip, profiles/r06_cu_mask_lab.txt: bits 0..7 = one CU in each XCC, bits 0..31 = four): 32 CUs
// per XCD.  An XCD cannot be switched OFF by the mask: one whose 32 bits are all zero runs on a fallback set (the 0x0f-bytes
// mask "XCDs 0-3 only" measured 256 CUs), so a lane is a slice [lo, hi) of the CUs of EVERY XCD -- which also keeps the
// workgroup id % 8 -> XCD placement the L2 warm-up workgroups and the tile maps assume.
int wm_cu_mask(int cu_lo, int cu_hi, uint32_t mask[8]) {
    for (int w = 0; w < 8; ++w) mask[w] = 0;
    int n = 0;
    for (int i = 0; i < 256; ++i) {
        const int cu = i >> 3;
        if (cu >= cu_lo && cu < cu_hi) { mask[i >> 5] |= 1u << (i & 31); ++n; }
    }
    return n;
}

static int ctx_new(int device, wm_ctx **out, int cu_lo = 0, int cu_hi = 32) {
    WM_REQUIRE(out != nullptr, WM_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int n = 0;
    WM_HIP(hipGetDeviceCount(&n));
    WM_REQUIRE(device >= 0 && device < n, WM_ERR_HIP, "device %d not present (%d visible)", device, n);
    WM_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    WM_HIP(hipGetDeviceProperties(&prop, device));
    WM_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, WM_ERR_HIP,
               "device %d is %s; this library contains gfx950 code only", device, prop.gcnArchName);
    wm_ctx *c = new wm_ctx();
    c->device = device;
    hipError_t se;
    if (cu_lo > 0 || cu_hi < 32) {   // a lane confined to the CUs [cu_lo, cu_hi) of every XCD
        uint32_t mask[8];
        c->n_cus = wm_cu_mask(cu_lo, cu_hi, mask);
        c->cu_lo = cu_lo;
        c->cu_hi = cu_hi;
        se = hipExtStreamCreateWithCUMask(&c->stream, 8, mask);
    } else {
        se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    }
    if (se != hipSuccess) {
        delete c;
        wm_set_error("hipStreamCreate failed: %s", hipGetErrorString(se));
        return WM_ERR_HIP;
    }
    int st = wm_frontend_init(&c->fe, c->stream);
    if (st != WM_OK) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return st;
    }
    *out = c;
    return WM_OK;
}

extern "C" int wm_create_frontend(int device, wm_ctx **out) { return ctx_new(device, out); }

extern "C" int wm_create(const wm_dims *dims, int device, wm_ctx **out) try {
    WM_REQUIRE(dims != nullptr, WM_ERR_INVALID, "null dims");
    WM_TRY(ctx_new(device, out));
    int st = wm_model_create(*out, dims);
    if (st != WM_OK) {
        wm_destroy(*out);
        *out = nullptr;
    }
    return st;
} WM_API_CATCH

extern "C" int wm_clone(wm_ctx *parent, wm_ctx **out) try {
    WM_REQUIRE(parent && out, WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(parent->model, WM_ERR_STATE, "clone: the parent context has no model");
    WM_TRY(ctx_new(parent->device, out));
    int st = wm_model_clone(*out, parent);
    if (st != WM_OK) {
        wm_destroy(*out);
        *out = nullptr;
    }
    return st;
} WM_API_CATCH

int wm_clone_cus(wm_ctx *parent, int cu_lo, int cu_hi, wm_ctx **out) {
    WM_REQUIRE(parent && out && parent->model, WM_ERR_INVALID, "clone_cus: bad arguments");
    WM_REQUIRE(cu_lo >= 0 && cu_lo < cu_hi && cu_hi <= 32, WM_ERR_INVALID, "clone_cus: CUs [%d, %d) of 32 per XCD", cu_lo, cu_hi);
    WM_TRY(ctx_new(parent->device, out, cu_lo, cu_hi));
    int st = wm_model_clone(*out, parent);
    if (st != WM_OK) {
        wm_destroy(*out);
        *out = nullptr;
    }
    return st;
}

extern "C" void wm_destroy(wm_ctx *ctx) {
    if (!ctx) return;
    // clones go before the weights they alias
    (void)wm_for_each_lane(ctx, false, [](wm_ctx *lane) { wm_destroy(lane); return (int)WM_OK; });
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    wm_model_destroy(ctx);
    wm_frontend_destroy(&ctx->fe);
    wm_resample_destroy(&ctx->rs);
    wm_vad_destroy(&ctx->vad);
    wm_chanact_destroy(&ctx->chanact);
    ctx->prof.reset();
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// ---------------------------------------------------------------- device helpers -----
extern "C" int wm_dev_malloc(wm_ctx *ctx, size_t bytes, void **dptr) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(dptr != nullptr, WM_ERR_INVALID, "null dptr");
    WM_HIP(hipMalloc(dptr, bytes ? bytes : 1));
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_dev_free(wm_ctx *ctx, void *dptr) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    if (dptr) WM_HIP(hipFree(dptr));
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_dev_upload(wm_ctx *ctx, void *dptr, const void *host, size_t bytes) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(dptr && host, WM_ERR_INVALID, "null pointer");
    WM_HIP(hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_dev_download(wm_ctx *ctx, void *host, const void *dptr, size_t bytes) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(dptr && host, WM_ERR_INVALID, "null pointer");
    WM_HIP(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_sync(wm_ctx *ctx) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// ---------------------------------------------------------------- profiling ABI ------
extern "C" int wm_profile_enable(wm_ctx *ctx, int on) try {
    WM_TRY(wm_ctx_make_current(ctx));
    ctx->prof.drain();
    ctx->prof.on = (on != 0);
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_profile_reset(wm_ctx *ctx) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->prof.reset();
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_profile_json(wm_ctx *ctx, char *buf, size_t n) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(buf && n > 2, WM_ERR_INVALID, "bad buffer");
    WM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->prof.drain();
    std::string s = "{";
    bool first = true;
    for (auto &kv : ctx->prof.fam) {
        char tmp[256];
        snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"ms\": %.6f, \"n\": %ld}", first ? "" : ", ",
                 kv.first.c_str(), kv.second.ms, kv.second.n);
        s += tmp;
        first = false;
    }
    s += "}";
    WM_REQUIRE(s.size() + 1 <= n, WM_ERR_INVALID, "buffer too small (%zu needed)", s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return WM_OK;
} WM_API_CATCH
// Cost of the measurement itself.  A kernel that spins for exactly T microseconds of the device
// clock is bracketed by the same two hipEventRecord calls the profiler uses, queued behind a long
// kernel so that the host runs ahead of the GPU (as it does in the real pipeline); the bias is the
// mean (elapsed - T): launch latency of a dependent kernel plus the completion of the closing event.
int wm_launch_spin(hipStream_t s, int *p, int grid, int cycles);
extern "C" int wm_profile_overhead_us(wm_ctx *ctx, float *us) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(us, WM_ERR_INVALID, "null pointer");
    WM_HIP(hipStreamSynchronize(ctx->stream));
    const int n = 64, spin_us = 15;
    std::vector<hipEvent_t> ev(2 * n);
    for (auto &e : ev) WM_HIP(hipEventCreate(&e));
    WM_TRY(wm_launch_spin(ctx->stream, nullptr, 160, 200000));  // 2 ms head start for the host
    for (int i = 0; i < n; ++i) {
        WM_HIP(hipEventRecord(ev[2 * i], ctx->stream));
        WM_TRY(wm_launch_spin(ctx->stream, nullptr, 160, spin_us * 100));  // wall_clock64: 100 MHz
        WM_HIP(hipEventRecord(ev[2 * i + 1], ctx->stream));
    }
    WM_HIP(hipStreamSynchronize(ctx->stream));
    double tot = 0;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        WM_HIP(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
        tot += ms;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    *us = (float)(tot * 1e3 / n) - (float)spin_us;
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_last_stage_ms(wm_ctx *ctx, float out3[3]) try {
    WM_REQUIRE(ctx && out3, WM_ERR_INVALID, "null pointer");
    for (int i = 0; i < 3; ++i) out3[i] = ctx->stage_ms[i];
    return WM_OK;
} WM_API_CATCH

// ---------------------------------------------------------------- boundary #1 --------
static int ensure_scratch(wm_ctx *ctx, size_t bytes) {
    if (ctx->fe.scratch_bytes >= bytes) return WM_OK;
    if (ctx->fe.scratch) WM_HIP(hipFree(ctx->fe.scratch));
    ctx->fe.scratch = nullptr;
    ctx->fe.scratch_bytes = 0;
    WM_HIP(hipMalloc(&ctx->fe.scratch, bytes));
    ctx->fe.scratch_bytes = bytes;
    return WM_OK;
}

static size_t dtype_size(wm_dtype t) {
    switch (t) {
        case WM_I16: return 2;
        case WM_F32: return 4;
        case WM_F64: return 8;
        case WM_BF16: return 2;
    }
    return 0;
}

// The MaximumLikelihoodRanker's score of one hypothesis: sum / n_text (an empty text counts as 1: the library's own rule
// where openai-whisper divides by zero), or sum / ((5 + n_text) / 6) ** length_penalty.  wm_rank_candidates and
// wm_transcribe_mel_beam's best_out.
double wm_rank_score(double sum, int n_text, float length_penalty) {
    double penalty;
    if (std::isnan(length_penalty)) penalty = n_text > 0 ? (double)n_text : 1.0;
    else penalty = pow((5.0 + (double)n_text) / 6.0, (double)length_penalty);
    return sum / penalty;
}

// openai-whisper's MaximumLikelihoodRanker (whisper/decoding.py): host only, no context, no GPU
extern "C" int wm_rank_candidates(const int32_t *tokens, const int32_t *lens, const float *token_logprobs, int B, int n_cand,
                                  int max_new, int32_t eot, float length_penalty, int32_t *best_out, double *score_out) try {
    WM_REQUIRE(tokens && lens && token_logprobs && best_out, WM_ERR_INVALID, "rank_candidates: null pointer");
    WM_REQUIRE(B >= 1 && n_cand >= 1 && max_new >= 1, WM_ERR_INVALID, "rank_candidates: B, n_cand and max_new must be >= 1");
    WM_REQUIRE(std::isnan(length_penalty) || (length_penalty >= 0.f && length_penalty <= 1.f), WM_ERR_INVALID,
               "rank_candidates: length_penalty must be NaN (none) or in [0, 1]");
    for (size_t i = 0; i < (size_t)B * n_cand; ++i)
        WM_REQUIRE(lens[i] >= 0 && lens[i] <= max_new, WM_ERR_INVALID, "rank_candidates: length %d of candidate %zu outside [0, %d]",
                   lens[i], i, max_new);
    for (int b = 0; b < B; ++b) {
        int best = 0;
        double best_score = -INFINITY;
        for (int s = 0; s < n_cand; ++s) {
            const size_t r = (size_t)b * n_cand + s;
            const int32_t *t = tokens + r * max_new;
            const float *lp = token_logprobs + r * max_new;
            double sum = 0.0;
            for (int i = 0; i < lens[r]; ++i) sum += (double)lp[i];
            int n_text = 0;
            while (n_text < lens[r] && t[n_text] != eot) ++n_text;
            const double score = wm_rank_score(sum, n_text, length_penalty);
            if (score_out) score_out[r] = score;
            if (score > best_score) { best_score = score; best = s; }   // the first maximal score; all -inf: candidate 0
        }
        best_out[b] = best;
    }
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_logmel(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int n_chunks,
                         int n_mels, void *out, wm_dtype out_dtype, wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(n_chunks >= 0, WM_ERR_INVALID, "n_chunks < 0");
    WM_REQUIRE(n_mels == 80 || n_mels == 128, WM_ERR_INVALID, "n_mels must be 80 or 128, got %d", n_mels);
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32 || pcm_dtype == WM_F64, WM_ERR_INVALID,
               "pcm dtype must be WM_I16 / WM_F32 / WM_F64");
    WM_REQUIRE(out_dtype == WM_F32 || out_dtype == WM_F64, WM_ERR_INVALID,
               "out dtype must be WM_F32 / WM_F64");
    if (n_chunks == 0) return WM_OK;
    WM_REQUIRE(pcm && out, WM_ERR_INVALID, "null pcm / out");
    if (mem == WM_MEM_DEVICE)
        return wm_frontend_run(&ctx->fe, &ctx->prof, ctx->stream, pcm, pcm_dtype, n_chunks, n_mels,
                               out, out_dtype);
    const size_t in_b = (size_t)n_chunks * WM_N_SAMPLES * dtype_size(pcm_dtype);
    const size_t out_b = (size_t)n_chunks * n_mels * WM_N_FRAMES * dtype_size(out_dtype);
    const size_t in_al = (in_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + out_b));
    char *d_in = (char *)ctx->fe.scratch, *d_out = d_in + in_al;
    WM_HIP(hipMemcpyAsync(d_in, pcm, in_b, hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_frontend_run(&ctx->fe, &ctx->prof, ctx->stream, d_in, pcm_dtype, n_chunks, n_mels,
                           d_out, out_dtype));
    WM_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_logmel_long(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *sample_offsets, int R,
                              int n_mels, float *out, wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "R must be 0 .. 65535, got %d", R);
    WM_REQUIRE(n_mels == 80 || n_mels == 128, WM_ERR_INVALID, "n_mels must be 80 or 128, got %d", n_mels);
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32 || pcm_dtype == WM_F64, WM_ERR_INVALID,
               "pcm dtype must be WM_I16 / WM_F32 / WM_F64");
    if (R == 0) return WM_OK;
    WM_REQUIRE(sample_offsets && out, WM_ERR_INVALID, "null sample_offsets / out");
    int64_t n_out = 0;
    for (int r = 0; r < R; ++r) {
        WM_REQUIRE(sample_offsets[r] >= 0 && sample_offsets[r + 1] >= sample_offsets[r], WM_ERR_INVALID,
                   "sample_offsets must be >= 0 and non-decreasing (recording %d)", r);
        n_out += (int64_t)n_mels * wm_long_frames(sample_offsets[r + 1] - sample_offsets[r]);
    }
    WM_REQUIRE(sample_offsets[R] == 0 || pcm, WM_ERR_INVALID, "null pcm");
    if (mem == WM_MEM_DEVICE)
        return wm_frontend_run_long(&ctx->fe, &ctx->prof, ctx->stream, pcm, pcm_dtype, sample_offsets, R, n_mels, out);
    // host memory: only the samples the recordings span cross PCIe (offsets rebased to the first one)
    std::vector<int64_t> offs(sample_offsets, sample_offsets + R + 1);
    for (auto &o : offs) o -= sample_offsets[0];
    const size_t in_b = (size_t)offs[R] * dtype_size(pcm_dtype);
    const size_t out_b = (size_t)n_out * sizeof(float);
    const size_t in_al = (in_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + out_b));
    char *d_in = (char *)ctx->fe.scratch, *d_out = d_in + in_al;
    if (in_b)
        WM_HIP(hipMemcpyAsync(d_in, (const char *)pcm + (size_t)sample_offsets[0] * dtype_size(pcm_dtype), in_b,
                              hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_frontend_run_long(&ctx->fe, &ctx->prof, ctx->stream, d_in, pcm_dtype, offs.data(), R, n_mels, (float *)d_out));
    WM_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// Recordings at any rate / channel count -> 16 kHz mono f32 (resample.hip), in wm_logmel_long's input layout
extern "C" int wm_resample_16k(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *elem_offsets,
                               const int32_t *n_channels, const int32_t *sample_rates, int R, float *out, wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "resample: R must be 0 .. 65535, got %d", R);
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32, WM_ERR_INVALID, "resample: pcm dtype must be WM_I16 / WM_F32");
    if (R == 0) return WM_OK;
    WM_REQUIRE(elem_offsets && n_channels && sample_rates, WM_ERR_INVALID, "resample: null elem_offsets / n_channels / sample_rates");
    int64_t n_out = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t len = elem_offsets[r + 1] - elem_offsets[r];
        WM_REQUIRE(elem_offsets[r] >= 0 && len >= 0, WM_ERR_INVALID, "resample: elem_offsets must be >= 0 and non-decreasing (recording %d)", r);
        WM_REQUIRE(n_channels[r] >= 1 && n_channels[r] <= WM_RS_MAX_CHANNELS, WM_ERR_INVALID,
                   "resample: recording %d: %d channels (1 .. %d)", r, n_channels[r], WM_RS_MAX_CHANNELS);
        WM_REQUIRE(len % n_channels[r] == 0, WM_ERR_INVALID, "resample: recording %d: %lld samples are no multiple of its %d channels",
                   r, (long long)len, n_channels[r]);
        const int64_t n = wm_resample_out_len(len / n_channels[r], sample_rates[r]);
        WM_REQUIRE(n >= 0, WM_ERR_INVALID, "resample: recording %d: unsupported sample rate %d", r, sample_rates[r]);
        n_out += n;
    }
    if (n_out == 0) return WM_OK;
    WM_REQUIRE(pcm && out, WM_ERR_INVALID, "resample: null pcm / out");
    if (mem == WM_MEM_DEVICE)
        return wm_resample_run(&ctx->rs, &ctx->prof, ctx->stream, pcm, pcm_dtype, elem_offsets, n_channels, sample_rates, R, out);
    // host memory: only the samples the recordings span cross PCIe (offsets rebased to the first one)
    std::vector<int64_t> offs(elem_offsets, elem_offsets + R + 1);
    for (auto &o : offs) o -= elem_offsets[0];
    const size_t in_b = (size_t)offs[R] * dtype_size(pcm_dtype);
    const size_t out_b = (size_t)n_out * sizeof(float);
    const size_t in_al = (in_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + out_b));
    char *d_in = (char *)ctx->fe.scratch, *d_out = d_in + in_al;
    WM_HIP(hipMemcpyAsync(d_in, (const char *)pcm + (size_t)elem_offsets[0] * dtype_size(pcm_dtype), in_b, hipMemcpyHostToDevice,
                          ctx->stream));
    WM_TRY(wm_resample_run(&ctx->rs, &ctx->prof, ctx->stream, d_in, pcm_dtype, offs.data(), n_channels, sample_rates, R, (float *)d_out));
    WM_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// wm_resample_16k with a channel matrix: n_rows[r] signals per recording, each in wm_logmel_long's input layout
extern "C" int wm_resample_16k_mix(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *elem_offsets,
                                   const int32_t *n_channels, const int32_t *sample_rates, int R, const int32_t *n_rows,
                                   const float *mix, float *out, wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "resample: R must be 0 .. 65535, got %d", R);
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32, WM_ERR_INVALID, "resample: pcm dtype must be WM_I16 / WM_F32");
    if (R == 0) return WM_OK;
    WM_REQUIRE(elem_offsets && n_channels && sample_rates, WM_ERR_INVALID, "resample: null elem_offsets / n_channels / sample_rates");
    WM_REQUIRE(n_rows && mix, WM_ERR_INVALID, "resample_mix: null n_rows / mix");
    int64_t n_out = 0, n_sig = 0;
    const float *w = mix;
    for (int r = 0; r < R; ++r) {
        const int64_t len = elem_offsets[r + 1] - elem_offsets[r];
        WM_REQUIRE(elem_offsets[r] >= 0 && len >= 0, WM_ERR_INVALID, "resample: elem_offsets must be >= 0 and non-decreasing (recording %d)", r);
        WM_REQUIRE(n_channels[r] >= 1 && n_channels[r] <= WM_RS_MAX_CHANNELS, WM_ERR_INVALID,
                   "resample: recording %d: %d channels (1 .. %d)", r, n_channels[r], WM_RS_MAX_CHANNELS);
        WM_REQUIRE(len % n_channels[r] == 0, WM_ERR_INVALID, "resample: recording %d: %lld samples are no multiple of its %d channels",
                   r, (long long)len, n_channels[r]);
        const int64_t n = wm_resample_out_len(len / n_channels[r], sample_rates[r]);
        WM_REQUIRE(n >= 0, WM_ERR_INVALID, "resample: recording %d: unsupported sample rate %d", r, sample_rates[r]);
        WM_REQUIRE(n_rows[r] >= 1 && n_rows[r] <= WM_RS_MAX_CHANNELS, WM_ERR_INVALID, "resample_mix: recording %d: %d rows (1 .. %d)", r,
                   n_rows[r], WM_RS_MAX_CHANNELS);
        n_sig += n_rows[r];
        WM_REQUIRE(n_sig <= 65535, WM_ERR_INVALID, "resample_mix: more than 65535 output signals");
        for (int i = 0; i < n_rows[r] * n_channels[r]; ++i, ++w)
            WM_REQUIRE(std::isfinite(*w), WM_ERR_INVALID, "resample_mix: recording %d: weight %d of its matrix is not finite", r, i);
        n_out += n * n_rows[r];
    }
    if (n_out == 0) return WM_OK;
    WM_REQUIRE(pcm && out, WM_ERR_INVALID, "resample: null pcm / out");
    if (mem == WM_MEM_DEVICE)
        return wm_resample_mix_run(&ctx->rs, &ctx->prof, ctx->stream, pcm, pcm_dtype, elem_offsets, n_channels, sample_rates, R, n_rows,
                                   mix, out);
    // host memory: only the samples the recordings span cross PCIe (offsets rebased to the first one)
    std::vector<int64_t> offs(elem_offsets, elem_offsets + R + 1);
    for (auto &o : offs) o -= elem_offsets[0];
    const size_t in_b = (size_t)offs[R] * dtype_size(pcm_dtype);
    const size_t out_b = (size_t)n_out * sizeof(float);
    const size_t in_al = (in_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + out_b));
    char *d_in = (char *)ctx->fe.scratch, *d_out = d_in + in_al;
    WM_HIP(hipMemcpyAsync(d_in, (const char *)pcm + (size_t)elem_offsets[0] * dtype_size(pcm_dtype), in_b, hipMemcpyHostToDevice,
                          ctx->stream));
    WM_TRY(wm_resample_mix_run(&ctx->rs, &ctx->prof, ctx->stream, d_in, pcm_dtype, offs.data(), n_channels, sample_rates, R, n_rows, mix,
                               (float *)d_out));
    WM_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// Per-channel activity of 16 kHz signals (channel_activity.hip): the sum of |y| per 160 samples
extern "C" int wm_channel_activity(wm_ctx *ctx, const float *pcm16k, const int64_t *sample_offsets, int S, float *act_out,
                                   wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(S >= 0 && S <= 65535, WM_ERR_INVALID, "channel_activity: S must be 0 .. 65535, got %d", S);
    if (S == 0) return WM_OK;
    WM_REQUIRE(sample_offsets, WM_ERR_INVALID, "channel_activity: null sample_offsets");
    int64_t n_out = 0;
    for (int s = 0; s < S; ++s) {
        WM_REQUIRE(sample_offsets[s] >= 0 && sample_offsets[s + 1] >= sample_offsets[s], WM_ERR_INVALID,
                   "channel_activity: sample_offsets must be >= 0 and non-decreasing (signal %d)", s);
        n_out += (sample_offsets[s + 1] - sample_offsets[s] + WM_ACTIVITY_HOP - 1) / WM_ACTIVITY_HOP;
    }
    if (n_out == 0) return WM_OK;
    WM_REQUIRE(pcm16k && act_out, WM_ERR_INVALID, "channel_activity: null pcm16k / act_out");
    if (mem == WM_MEM_DEVICE) return wm_chanact_run(&ctx->chanact, &ctx->prof, ctx->stream, pcm16k, sample_offsets, S, act_out);
    // host memory: only the samples the signals span cross PCIe (offsets rebased to the first one)
    std::vector<int64_t> offs(sample_offsets, sample_offsets + S + 1);
    for (auto &o : offs) o -= sample_offsets[0];
    const size_t in_b = (size_t)offs[S] * sizeof(float), out_b = (size_t)n_out * sizeof(float);
    const size_t in_al = (in_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + out_b));
    char *d_in = (char *)ctx->fe.scratch, *d_out = d_in + in_al;
    WM_HIP(hipMemcpyAsync(d_in, pcm16k + sample_offsets[0], in_b, hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_chanact_run(&ctx->chanact, &ctx->prof, ctx->stream, (const float *)d_in, offs.data(), S, (float *)d_out));
    WM_HIP(hipMemcpyAsync(act_out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// Speech-activity energy of wm_logmel_long's output (vad.hip): per frame, log10 of the band's mel power, smoothed
extern "C" int wm_vad_energy(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len, const int32_t *n_frames,
                             int R, int n_mels, int band_lo, int band_hi, int smooth, float *raw_out, float *energy_out,
                             wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "vad: R must be 0 .. 65535, got %d", R);
    WM_REQUIRE(n_mels == 80 || n_mels == 128, WM_ERR_INVALID, "vad: n_mels must be 80 or 128, got %d", n_mels);
    WM_REQUIRE(band_lo >= 0 && band_lo < band_hi && band_hi <= n_mels, WM_ERR_INVALID, "vad: band [%d, %d) outside 0 <= lo < hi <= %d",
               band_lo, band_hi, n_mels);
    WM_REQUIRE(smooth >= 1 && smooth <= WM_VAD_MAX_SMOOTH && (smooth & 1), WM_ERR_INVALID, "vad: smooth must be odd, 1 .. %d, got %d",
               WM_VAD_MAX_SMOOTH, smooth);
    if (R == 0) return WM_OK;
    WM_REQUIRE(mel && mel_base && mel_len && n_frames && energy_out, WM_ERR_INVALID, "vad: null pointer");
    const int n_band = band_hi - band_lo;
    std::vector<int64_t> row0(R);
    int64_t n_out = 0, n_in = 0;
    for (int r = 0; r < R; ++r) {
        WM_REQUIRE(mel_base[r] >= 0 && mel_len[r] >= 1, WM_ERR_INVALID, "vad: recording %d: mel_base %lld, mel_len %d", r,
                   (long long)mel_base[r], mel_len[r]);
        WM_REQUIRE(n_frames[r] >= 0 && n_frames[r] <= mel_len[r], WM_ERR_INVALID, "vad: recording %d: n_frames %d outside [0, %d]", r,
                   n_frames[r], mel_len[r]);
        row0[r] = mem == WM_MEM_DEVICE ? mel_base[r] + (int64_t)band_lo * mel_len[r] : n_in;
        n_out += n_frames[r];
        n_in += (int64_t)n_band * mel_len[r];
    }
    if (mem == WM_MEM_DEVICE)
        return wm_vad_run(&ctx->vad, &ctx->prof, ctx->stream, mel, row0.data(), mel_len, n_frames, R, n_band, smooth, raw_out, energy_out);
    if (n_out == 0) return WM_OK;
    // host memory: only each recording's band rows cross PCIe, packed one recording after the other
    const size_t in_b = (size_t)n_in * sizeof(float), out_b = (size_t)n_out * sizeof(float);
    const size_t in_al = (in_b + 255) & ~(size_t)255, out_al = (out_b + 255) & ~(size_t)255;
    WM_TRY(ensure_scratch(ctx, in_al + 2 * out_al));
    char *d_in = (char *)ctx->fe.scratch, *d_y = d_in + in_al, *d_raw = d_y + out_al;
    for (int r = 0; r < R; ++r)
        WM_HIP(hipMemcpyAsync(d_in + (size_t)row0[r] * sizeof(float), mel + mel_base[r] + (int64_t)band_lo * mel_len[r],
                              (size_t)n_band * mel_len[r] * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_vad_run(&ctx->vad, &ctx->prof, ctx->stream, (const float *)d_in, row0.data(), mel_len, n_frames, R, n_band, smooth,
                      raw_out ? (float *)d_raw : nullptr, (float *)d_y));
    WM_HIP(hipMemcpyAsync(energy_out, d_y, out_b, hipMemcpyDeviceToHost, ctx->stream));
    if (raw_out) WM_HIP(hipMemcpyAsync(raw_out, d_raw, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// The reference's symbol (bridge.h:11 / lib.rs:110-122).  The Rust crate's entry is re-entrant (immutable lazily
// initialised state, lib.rs:11-14), so concurrent callers must not queue behind one another here either: a small pool of
// lazily created front-end contexts (own stream, tables and staging each), handed out under a mutex and used outside it.
// At most kGsMaxContexts (8) callers run concurrently -- a ninth waits for a context to come back --; the contexts live
// for the rest of the process (the symbol has no teardown counterpart in the reference's ABI either: bridge.h declares
// one function), a few MB of HBM each; $WM_DEVICE is read once, when the first context is made.
namespace {
constexpr int kGsMaxContexts = 8;
std::mutex g_gs_mutex;
std::condition_variable g_gs_cv;
std::vector<wm_ctx *> g_gs_free;
int g_gs_created = 0;

wm_ctx *gs_acquire() {
    {
        std::unique_lock<std::mutex> lock(g_gs_mutex);
        for (;;) {
            if (!g_gs_free.empty()) {
                wm_ctx *c = g_gs_free.back();
                g_gs_free.pop_back();
                return c;
            }
            if (g_gs_created < kGsMaxContexts) {
                ++g_gs_created;
                break;  // create one outside the lock
            }
            g_gs_cv.wait(lock);
        }
    }
    static const int device = [] {
        const char *dev = getenv("WM_DEVICE");
        return dev ? atoi(dev) : 0;
    }();
    wm_ctx *c = nullptr;
    if (wm_create_frontend(device, &c) != WM_OK) {
        fprintf(stderr, "generate_spectrogram: no usable MI355X context (%s); there is no CPU fallback\n", wm_last_error());
        abort();  // the reference panics (=abort across FFI) on its internal failures too
    }
    return c;
}

void gs_release(wm_ctx *c) {
    {
        std::lock_guard<std::mutex> lock(g_gs_mutex);
        g_gs_free.push_back(c);
    }
    g_gs_cv.notify_one();
}
}  // namespace

extern "C" void generate_spectrogram(double *audio, double *output) {
    // lib.rs:34-40,113: the reflect pad is written into the CALLER's buffer (visible side effect).
    for (int i = 0; i < 200; ++i) {
        audio[i] = audio[400 - i];
        const int j = 16000 * 30 + i + 200;
        audio[j] = audio[200 + (16000 * 30 - 2) - i];
    }
    wm_ctx *ctx = gs_acquire();
    // The device kernel re-derives the same pad by index arithmetic from samples [200, 480200).
    int st = wm_logmel(ctx, audio + 200, WM_F64, 1, 80, output, WM_F64, WM_MEM_HOST);
    if (st != WM_OK) {
        fprintf(stderr, "generate_spectrogram: %s\n", wm_last_error());
        abort();
    }
    gs_release(ctx);
}
