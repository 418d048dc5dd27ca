// vad.hip -- speech-activity energy of whole-recording log-mels on the device: the kernel and its
// device-pointer core.  The C-ABI entry wm_vad_energy is in api.cpp beside wm_resample_16k; the host-only segment rule
// (wm_vad_segments) is in vad_segments.cpp.
//
// Input: wm_logmel_long's output, recording r = [n_mels][T_r] at element base_r, v = (max(log10 mel, gmax_r - 8) + 4) / 4.
// For frame t < n_r <= T_r over the band rows m in [lo, hi):
//     vmax = max_m v[m][t],   s = sum_m exp2f((v[m][t] - vmax) * (4 log2 10))   (f32, m ascending)
//     e[t] = 4 vmax + log10f(s)                                                 (log10 of the band's mel power, + 4)
//     y[t] = (sum_{u = max(0, t - h)}^{min(n - 1, t + h)} e[u]) * (1.0f / count),  h = smooth / 2   (f32, u ascending)
// Both orders are functions of (recording, t) alone -- never of the tile, the lane or the grid -- so a recording's output is
// bit-identical alone, among others and at any base.
#include <math.h>

#include "wm_internal.h"

namespace {
constexpr int VAD_THREADS = 256;
constexpr int VAD_MAX_H = WM_VAD_MAX_SMOOTH / 2;          // 15
constexpr int VAD_TILE = VAD_THREADS - 2 * (VAD_MAX_H + 1);   // 224 frames per workgroup: tile + both halos = one lane each

struct VadRec {
    long long base;   // element of v[lo][0]: the band's first row
    long long out;    // first output element of the recording (packed)
    int T;            // row stride (frames of the block)
    int n;            // frames to do
};
static_assert(sizeof(VadRec) == 24, "VadRec is copied to the device as is");

// One workgroup per (recording, tile of VAD_TILE consecutive frames).  Lane i owns frame u = t0 - h + i of the tile and its
// halo: it walks the band rows twice (the maximum, then the sum; the second walk hits L2), every row read coalesced along
// t, and leaves e[u] in LDS.  Lanes h .. h + VAD_TILE - 1 then smooth their frame from LDS.
__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const float *__restrict__ mel, const VadRec *__restrict__ recs,
                                                                 const int2 *__restrict__ blks, int n_band, int h,
                                                                 float *__restrict__ raw, float *__restrict__ out) {
    __shared__ float e_lds[VAD_THREADS];
    const int2 b = blks[blockIdx.x];
    const VadRec rc = recs[b.x];
    const int t0 = b.y, i = threadIdx.x;
    const int u = t0 - h + i;
    const bool own = i >= h && i < h + VAD_TILE && u < rc.n;   // a frame of the tile itself
    if (i < VAD_TILE + 2 * h && u >= 0 && u < rc.n) {
        const float *col = mel + rc.base + u;
        float vmax = col[0];
        for (int m = 1; m < n_band; ++m) {
            const float v = col[(long long)m * rc.T];
            vmax = (v > vmax || v != v) ? v : vmax;   // a NaN stays
        }
        float s = 0.f;
        for (int m = 0; m < n_band; ++m) s += exp2f((col[(long long)m * rc.T] - vmax) * 13.287712379549449f);
        const float e = 4.f * vmax + log10f(s);
        e_lds[i] = e;
        if (raw != nullptr && own) raw[rc.out + u] = e;
    }
    __syncthreads();
    if (own) {
        const int a = u - h > 0 ? u - h : 0, z = u + h < rc.n - 1 ? u + h : rc.n - 1;   // both inside [t0 - h, t0 + VAD_TILE + h)
        float acc = 0.f;
        for (int w = a; w <= z; ++w) acc += e_lds[w - (t0 - h)];
        out[rc.out + u] = acc * (1.0f / (float)(z - a + 1));
    }
}
}  // namespace

void wm_vad_destroy(WmVad *vad) {
    if (vad->tab) (void)hipFree(vad->tab);
    *vad = WmVad();
}

int wm_vad_run(WmVad *vad, WmProfiler *prof, hipStream_t stream, const float *d_mel, const int64_t *row0, const int32_t *stride,
               const int32_t *n_frames, int R, int n_band, int smooth, float *d_raw, float *d_energy) {
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "vad: R must be 0 .. 65535, got %d", R);
    WM_REQUIRE(n_band >= 1 && n_band <= 128, WM_ERR_INVALID, "vad: band of %d rows (1 .. 128)", n_band);
    WM_REQUIRE(smooth >= 1 && smooth <= WM_VAD_MAX_SMOOTH && (smooth & 1), WM_ERR_INVALID, "vad: smooth must be odd, 1 .. %d, got %d",
               WM_VAD_MAX_SMOOTH, smooth);
    if (R == 0) return WM_OK;
    WM_REQUIRE(row0 && stride && n_frames, WM_ERR_INVALID, "vad: null mel_base / mel_len / n_frames");
    std::vector<VadRec> rec(R);
    std::vector<int2> blk;
    long long out = 0;
    for (int r = 0; r < R; ++r) {
        WM_REQUIRE(row0[r] >= 0 && stride[r] >= 1 && n_frames[r] >= 0 && n_frames[r] <= stride[r], WM_ERR_INVALID,
                   "vad: recording %d: base %lld, %d frames of a block of %d", r, (long long)row0[r], n_frames[r], stride[r]);
        rec[r] = VadRec{row0[r], out, stride[r], n_frames[r]};
        out += n_frames[r];
        for (int t0 = 0; t0 < n_frames[r]; t0 += VAD_TILE) blk.push_back(make_int2(r, t0));
    }
    if (blk.empty()) return WM_OK;
    WM_REQUIRE(blk.size() < ((size_t)1 << 24), WM_ERR_INVALID, "vad: %zu tiles of %d frames in one call (at most 2^24 - 1)", blk.size(),
               VAD_TILE);
    WM_REQUIRE(d_mel && d_energy, WM_ERR_INVALID, "vad: null mel / energy_out");
    const size_t rec_b = (sizeof(VadRec) * R + 255) & ~(size_t)255, bytes = rec_b + sizeof(int2) * blk.size();
    if (vad->tab_bytes < bytes) {
        WM_HIP(hipStreamSynchronize(stream));
        if (vad->tab) WM_HIP(hipFree(vad->tab));
        vad->tab = nullptr;
        vad->tab_bytes = 0;
        WM_HIP(hipMalloc(&vad->tab, bytes));
        vad->tab_bytes = bytes;
    }
    const VadRec *d_rec = (const VadRec *)vad->tab;
    const int2 *d_blk = (const int2 *)((char *)vad->tab + rec_b);
    WM_HIP(hipMemcpyAsync(vad->tab, rec.data(), sizeof(VadRec) * R, hipMemcpyHostToDevice, stream));
    WM_HIP(hipMemcpyAsync((void *)d_blk, blk.data(), sizeof(int2) * blk.size(), hipMemcpyHostToDevice, stream));
    {
        WmProfScope ps(prof, "vad", stream);
        vad_energy_kernel<<<(unsigned)blk.size(), VAD_THREADS, 0, stream>>>(d_mel, d_rec, d_blk, n_band, smooth / 2, d_raw, d_energy);
    }
    WM_HIP(hipGetLastError());
    // the tables are pageable host memory: the copies must have read them before they go out of scope
    WM_HIP(hipStreamSynchronize(stream));
    return WM_OK;
}
