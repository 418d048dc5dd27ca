// streams.hip -- the two small kernels of a set of live audio streams (wm_streams, streams.h) beside the stream rule of
// frontend.hip's stage-1 kernel:
//   streams_carry  : after a push's stage-1 launch has read the old carry, stream s's carry becomes the staged f32 samples
//                    that its frames which are not final still need: a slice of [old carry | new samples], at most 399 values.
//                    One workgroup per stream reads its whole slice into registers before it stores any of it, so the
//                    overlap of source and destination is harmless.
//   streams_window : row r = frames [first, first + n) of a stream, normalised as a recording that is the window:
//                    gmax = the maximum of the row's n per-frame maxima, found by every workgroup of the row on its own (at
//                    most 12 KB of reads) -- no atomics, one launch for all rows, deterministic; then
//                    (max(raw, gmax - 8) + 4) / 4 by clamp_affine, the arithmetic of logmel_stage2, with the ring unwrapped.
#include "streams.h"
#include "logmel_shared.h"

namespace {

constexpr int CARRY_T = 256;
static_assert(2 * CARRY_T >= WM_STREAM_CARRY, "two values per thread hold a whole carry");

__global__ __launch_bounds__(CARRY_T) void streams_carry(const void *__restrict__ pcm, int pcm_dtype,
                                                         const WmStreamRec *__restrict__ rec, float *__restrict__ carry_all) {
    const WmStreamRec r = rec[blockIdx.x];
    if (r.n_new == 0) return;   // (workgroup-uniform)
    float *carry = carry_all + (size_t)blockIdx.x * WM_STREAM_CARRY;
    float v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = u * CARRY_T + threadIdx.x;
        const int src = r.shift + t;   // index into [carry | new samples]
        float x = 0.f;
        if (t < r.new_len) {
            if (src < r.carry_len) x = carry[src];
            else if (src - r.carry_len < r.n_new) x = load_sample<float>(pcm, pcm_dtype, (size_t)r.pcm_base + (size_t)(src - r.carry_len));
        }
        v[u] = x;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = u * CARRY_T + threadIdx.x;
        if (t < r.new_len && t < WM_STREAM_CARRY) carry[t] = v[u];
    }
}

__global__ __launch_bounds__(256) void streams_window(const float *__restrict__ ring, const float *__restrict__ fmax, int n_mels, int cap,
                                                      const WmStreamWin *__restrict__ rows, float *__restrict__ out) {
    __shared__ float red[4];
    const WmStreamWin w = rows[blockIdx.y];
    const int tid = threadIdx.x;
    const float *fm = fmax + (size_t)w.stream * cap;
    float g = -1e30f;
    for (int i = tid; i < w.n; i += 256) {
        int c = w.col0 + i;
        if (c >= cap) c -= cap;
        const float v = fm[c];
        g = (v > g) ? v : g;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(g, off);
        g = (o > g) ? o : g;
    }
    if ((tid & 63) == 0) red[tid >> 6] = g;
    __syncthreads();
    g = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) g = (red[i] > g) ? red[i] : g;
    const unsigned long long gm = enc_max(g);
    const float *src = ring + (size_t)w.stream * n_mels * cap;
    float *dst = out + w.out_base;
    const int total = n_mels * w.n;   // <= 128 * 3000
    for (int idx = blockIdx.x * 256 + tid; idx < total; idx += gridDim.x * 256) {
        const int m = idx / w.n, t = idx - m * w.n;
        int c = w.col0 + t;
        if (c >= cap) c -= cap;
        dst[idx] = clamp_affine(src[(size_t)m * cap + c], gm);
    }
}

}  // namespace

int wm_streams_carry_run(hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype, const WmStreamRec *d_rec, float *d_carry, int S) {
    streams_carry<<<S, CARRY_T, 0, stream>>>(d_pcm, (int)pcm_dtype, d_rec, d_carry);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_streams_window_run(WmProfiler *prof, hipStream_t stream, const float *d_ring, const float *d_fmax, int n_mels, int cap,
                          const WmStreamWin *d_rows, int R, int max_n, float *d_out) {
    WmProfScope ps(prof, "streams_window", stream);
    int gx = (n_mels * max_n + 2047) / 2048;   // 8 values per thread at the longest row
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    streams_window<<<dim3(gx, R), 256, 0, stream>>>(d_ring, d_fmax, n_mels, cap, d_rows, d_out);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
