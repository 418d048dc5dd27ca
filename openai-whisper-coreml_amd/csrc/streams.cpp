// streams.cpp -- the C ABI of a set of live audio streams (include/whisper_mi355x.h, wm_streams_*): appended samples become
// log-mel frames incrementally on the device, and any window of the frames a stream still holds is normalised on demand.
// The frame arithmetic and the object are in streams.h, the kernels in frontend.hip (stage 1, the stream rule) and streams.hip
// (carry, window).  All sample and frame positions are 64-bit here and relative to the carry / the ring on the device.
#include <string.h>

#include <algorithm>
#include <vector>

#include "streams.h"

int g_wm_stream_min_capacity = WM_STREAM_MIN_CAPACITY;

namespace {

size_t pcm_size(wm_dtype t) { return t == WM_I16 ? 2 : (t == WM_F32 ? 4 : 8); }

int grow(hipStream_t stream, void **p, size_t *have, size_t want) {
    if (*have >= want) return WM_OK;
    WM_HIP(hipStreamSynchronize(stream));
    if (*p) WM_HIP(hipFree(*p));
    *p = nullptr;
    *have = 0;
    WM_HIP(hipMalloc(p, want));
    *have = want;
    return WM_OK;
}

// frames of stream s that a window may name: [first_kept, avail)
int64_t avail_of(const wm_streams *st, int s) { return st->stale[s] ? wm_stream_final(st->n[s]) : wm_stream_avail(st->n[s]); }
int64_t kept_of(const wm_streams *st, int s) {
    return std::max<int64_t>(std::max<int64_t>(0, avail_of(st, s) - st->cap), std::min(st->floor[s], avail_of(st, s)));
}

int check_set(const wm_ctx *ctx, const wm_streams *st) {
    WM_REQUIRE(st != nullptr, WM_ERR_INVALID, "streams: null set");
    WM_REQUIRE(st->device == ctx->device, WM_ERR_STATE, "streams: the set lives on device %d, the context on device %d", st->device,
               ctx->device);
    return WM_OK;
}

void destroy(wm_streams *st) {
    void *ptrs[] = {st->ring, st->fmax, st->carry, st->tab, st->stage};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete st;
}

}  // namespace

extern "C" int wm_streams_create(wm_ctx *ctx, int S, int n_mels, int capacity_frames, wm_streams **out) try {
    WM_REQUIRE(out != nullptr, WM_ERR_INVALID, "streams: null out pointer");
    *out = nullptr;
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(S >= 1 && S <= 65535, WM_ERR_INVALID, "streams: S must be 1 .. 65535, got %d", S);
    WM_REQUIRE(n_mels == 80 || n_mels == 128, WM_ERR_INVALID, "n_mels must be 80 or 128, got %d", n_mels);
    WM_REQUIRE(capacity_frames >= g_wm_stream_min_capacity, WM_ERR_INVALID, "streams: capacity_frames must be >= %d, got %d",
               g_wm_stream_min_capacity, capacity_frames);
    WM_REQUIRE((int64_t)S * n_mels * capacity_frames <= (int64_t)1 << 40, WM_ERR_INVALID, "streams: ring of %d x %d x %d values too large",
               S, n_mels, capacity_frames);
    wm_streams *st = new wm_streams();
    st->device = ctx->device;
    st->S = S;
    st->n_mels = n_mels;
    st->cap = capacity_frames;
    st->n.assign(S, 0);
    st->floor.assign(S, 0);
    st->reflect.assign(S, 1);
    st->stale.assign(S, 0);
    const size_t ring_b = sizeof(float) * S * n_mels * capacity_frames, fmax_b = sizeof(float) * S * capacity_frames,
                 carry_b = sizeof(float) * S * WM_STREAM_CARRY;
    hipError_t e = hipMalloc((void **)&st->ring, ring_b);
    if (e == hipSuccess) e = hipMalloc((void **)&st->fmax, fmax_b);
    if (e == hipSuccess) e = hipMalloc((void **)&st->carry, carry_b);
    // a window never reads a column that no push wrote; the rings start defined all the same
    if (e == hipSuccess) e = hipMemsetAsync(st->ring, 0, ring_b, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(st->fmax, 0, fmax_b, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(st->carry, 0, carry_b, ctx->stream);
    if (e != hipSuccess) {
        wm_set_error("streams: allocating %zu bytes failed: %s", ring_b + fmax_b + carry_b, hipGetErrorString(e));
        destroy(st);
        return e == hipErrorOutOfMemory ? WM_ERR_NOMEM : WM_ERR_HIP;
    }
    *out = st;
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_streams_free(wm_ctx *ctx, wm_streams *st) try {
    if (!st) return WM_OK;
    WM_TRY(wm_ctx_make_current(ctx));
    WM_TRY(check_set(ctx, st));
    WM_HIP(hipStreamSynchronize(ctx->stream));   // launches that read the set have ended
    destroy(st);
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_streams_reset(wm_ctx *ctx, wm_streams *st, int s) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_TRY(check_set(ctx, st));
    WM_REQUIRE(s >= 0 && s < st->S, WM_ERR_INVALID, "streams: stream %d outside 0 .. %d", s, st->S - 1);
    st->n[s] = 0;
    st->floor[s] = 0;
    st->reflect[s] = 1;
    st->stale[s] = 0;
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_streams_frames(const wm_streams *st, int64_t *samples, int64_t *final_frames, int64_t *avail_frames,
                                 int64_t *first_kept) try {
    WM_REQUIRE(st != nullptr, WM_ERR_INVALID, "streams: null set");
    for (int s = 0; s < st->S; ++s) {
        if (samples) samples[s] = st->n[s];
        if (final_frames) final_frames[s] = wm_stream_final(st->n[s]);
        if (avail_frames) avail_frames[s] = avail_of(st, s);
        if (first_kept) first_kept[s] = kept_of(st, s);
    }
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_streams_push(wm_ctx *ctx, wm_streams *st, const void *pcm, wm_dtype pcm_dtype, const int64_t *sample_offsets,
                               wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_TRY(check_set(ctx, st));
    WM_REQUIRE(sample_offsets != nullptr, WM_ERR_INVALID, "streams: null sample_offsets");
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32 || pcm_dtype == WM_F64, WM_ERR_INVALID,
               "pcm dtype must be WM_I16 / WM_F32 / WM_F64");
    WM_REQUIRE(mem == WM_MEM_HOST || mem == WM_MEM_DEVICE, WM_ERR_INVALID, "streams: bad mem space %d", (int)mem);
    const int S = st->S;
    WM_REQUIRE(sample_offsets[0] >= 0, WM_ERR_INVALID, "streams: sample_offsets must be >= 0");
    for (int s = 0; s < S; ++s) {
        const int64_t len = sample_offsets[s + 1] - sample_offsets[s];
        WM_REQUIRE(len >= 0 && len <= (int64_t)1 << 30, WM_ERR_INVALID,
                   "streams: stream %d: offsets [%lld, %lld) invalid (0 .. 2^30 samples per stream and call)", s,
                   (long long)sample_offsets[s], (long long)sample_offsets[s + 1]);
    }
    const int64_t total = sample_offsets[S] - sample_offsets[0];
    WM_REQUIRE(total == 0 || pcm, WM_ERR_INVALID, "streams: null pcm");
    // the tables: a record per stream, a workgroup per (stream, up to 64 frames) of the frames that became final and the
    // provisional ones -- of a push that brings more than the ring holds, only the frames that stay
    const int64_t rebase = mem == WM_MEM_HOST ? sample_offsets[0] : 0;
    std::vector<WmStreamRec> rec(S);
    std::vector<int4> blk;
    bool any_new = false;
    for (int s = 0; s < S; ++s) {
        const int64_t n_new = sample_offsets[s + 1] - sample_offsets[s];
        WmStreamRec &r = rec[s];
        memset(&r, 0, sizeof(r));
        if (n_new == 0 && !st->stale[s]) continue;
        const int64_t N0 = st->n[s], N1 = N0 + n_new;
        const int64_t c0 = wm_stream_carry_start(N0), c1 = wm_stream_carry_start(N1);
        r.pcm_base = sample_offsets[s] - rebase;
        r.carry_len = (int)(N0 - c0);
        r.n_new = (int)n_new;
        r.reflect = st->reflect[s];
        r.shift = (int)(c1 - c0);
        r.new_len = (int)(N1 - c1);
        any_new = any_new || n_new > 0;
        const int64_t A1 = wm_stream_avail(N1);
        const int64_t lo = std::max(std::max(wm_stream_final(N0), A1 - st->cap), st->floor[s]);
        for (int64_t f = lo; f < A1; f += WM_STREAM_FPB)
            blk.push_back(make_int4(s, (int)(f * WM_HOP - 200 - c0), (int)(f % st->cap), (int)std::min<int64_t>(WM_STREAM_FPB, A1 - f)));
    }
    WM_REQUIRE(blk.size() <= (size_t)0x7fffffff, WM_ERR_INVALID, "streams: %zu workgroups in one push", blk.size());
    if (blk.empty() && !any_new) return WM_OK;
    const size_t rec_b = (sizeof(WmStreamRec) * S + 255) & ~(size_t)255, bytes = rec_b + sizeof(int4) * std::max<size_t>(blk.size(), 1);
    WM_TRY(grow(ctx->stream, &st->tab, &st->tab_bytes, bytes));
    const void *d_pcm = pcm;
    if (mem == WM_MEM_HOST && total > 0) {   // only the named range crosses PCIe
        const size_t in_b = (size_t)total * pcm_size(pcm_dtype);
        WM_TRY(grow(ctx->stream, &st->stage, &st->stage_bytes, in_b));
        WM_HIP(hipMemcpyAsync(st->stage, (const char *)pcm + (size_t)sample_offsets[0] * pcm_size(pcm_dtype), in_b, hipMemcpyHostToDevice,
                              ctx->stream));
        d_pcm = st->stage;
    }
    WmStreamTab tab;
    tab.rec = (const WmStreamRec *)st->tab;
    tab.blk = (const int4 *)((char *)st->tab + rec_b);
    tab.carry = st->carry;
    tab.fmax = st->fmax;
    tab.cap = st->cap;
    WM_HIP(hipMemcpyAsync(st->tab, rec.data(), sizeof(WmStreamRec) * S, hipMemcpyHostToDevice, ctx->stream));
    if (!blk.empty())
        WM_HIP(hipMemcpyAsync((void *)tab.blk, blk.data(), sizeof(int4) * blk.size(), hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_frontend_run_stream(&ctx->fe, &ctx->prof, ctx->stream, d_pcm, pcm_dtype, st->n_mels, tab, (int)blk.size(), st->ring));
    if (any_new) WM_TRY(wm_streams_carry_run(ctx->stream, d_pcm, pcm_dtype, tab.rec, st->carry, S));
    // the tables and a host caller's samples are pageable memory: the copies must have read them before this returns
    WM_HIP(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < S; ++s) {
        st->n[s] += sample_offsets[s + 1] - sample_offsets[s];
        if (rec[s].n_new > 0 || st->stale[s]) st->stale[s] = 0;
    }
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_streams_window(wm_ctx *ctx, wm_streams *st, int R, const int32_t *stream, const int64_t *first_frame,
                                 const int32_t *n_frames, float *out, const int64_t *out_base, wm_mem mem) try {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_TRY(check_set(ctx, st));
    WM_REQUIRE(R >= 1 && R <= 65535, WM_ERR_INVALID, "streams: R must be 1 .. 65535, got %d", R);
    WM_REQUIRE(stream && first_frame && n_frames && out && out_base, WM_ERR_INVALID, "streams: null pointer");
    WM_REQUIRE(mem == WM_MEM_HOST || mem == WM_MEM_DEVICE, WM_ERR_INVALID, "streams: bad mem space %d", (int)mem);
    std::vector<WmStreamWin> rows(R);
    int max_n = 0;
    int64_t packed = 0;
    for (int r = 0; r < R; ++r) {
        const int s = stream[r];
        WM_REQUIRE(s >= 0 && s < st->S, WM_ERR_INVALID, "streams: row %d: stream %d outside 0 .. %d", r, s, st->S - 1);
        const int n = n_frames[r];
        WM_REQUIRE(n >= 1 && n <= WM_STREAM_MAX_WINDOW, WM_ERR_INVALID, "streams: row %d: n_frames must be 1 .. %d, got %d", r,
                   WM_STREAM_MAX_WINDOW, n);
        const int64_t K = kept_of(st, s), A = avail_of(st, s), f = first_frame[r];
        WM_REQUIRE(f >= K && f <= A - n, WM_ERR_INVALID, "streams: row %d: frames [%lld, %lld) outside the kept frames [%lld, %lld) of stream %d",
                   r, (long long)f, (long long)f + n, (long long)K, (long long)A, s);
        WM_REQUIRE(out_base[r] >= 0, WM_ERR_INVALID, "streams: row %d: negative out_base", r);
        rows[r].out_base = mem == WM_MEM_HOST ? packed : out_base[r];
        rows[r].stream = s;
        rows[r].col0 = (int)(f % st->cap);
        rows[r].n = n;
        rows[r].pad = 0;
        packed += (int64_t)st->n_mels * n;
        max_n = std::max(max_n, n);
    }
    const size_t row_b = (sizeof(WmStreamWin) * R + 255) & ~(size_t)255;
    float *d_out = out;
    const WmStreamWin *d_rows;
    if (mem == WM_MEM_HOST) {   // rows and the packed blocks in the set's staging buffer
        WM_TRY(grow(ctx->stream, &st->stage, &st->stage_bytes, row_b + sizeof(float) * (size_t)packed));
        d_rows = (const WmStreamWin *)st->stage;
        d_out = (float *)((char *)st->stage + row_b);
    } else {
        WM_TRY(grow(ctx->stream, &st->tab, &st->tab_bytes, row_b));
        d_rows = (const WmStreamWin *)st->tab;
    }
    WM_HIP(hipMemcpyAsync((void *)d_rows, rows.data(), sizeof(WmStreamWin) * R, hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(wm_streams_window_run(&ctx->prof, ctx->stream, st->ring, st->fmax, st->n_mels, st->cap, d_rows, R, max_n, d_out));
    if (mem == WM_MEM_HOST)
        for (int r = 0; r < R; ++r)
            WM_HIP(hipMemcpyAsync(out + out_base[r], d_out + rows[r].out_base, sizeof(float) * st->n_mels * rows[r].n,
                                  hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));   // the row table is pageable memory
    return WM_OK;
} WM_API_CATCH
