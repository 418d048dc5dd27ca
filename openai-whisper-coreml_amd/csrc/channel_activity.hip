// channel_activity.hip -- per-channel activity of 16 kHz signals on the device: the kernel and its
// device-pointer core.  The C-ABI entry wm_channel_activity is in api.cpp beside wm_resample_16k_mix, whose output layout
// this reads.
//
// Signal s of N samples y gets ceil(N / 160) values: act[f] = sum |y[160 f + i]| over i < 160 with 160 f + i < N (f32).
// THE ORDER of a frame's sum, a function of the frame alone:
//     p[j] = ((..(|y[j]| + |y[16 + j]|) + ..) + |y[144 + j]|)            j = 0 .. 15: ten terms, ascending, a missing term is +0
//     q[j] = p[j] + p[j + 8],  r[j] = q[j] + q[j + 4],  t[j] = r[j] + r[j + 2],  act = t[0] + t[1]
// Sixteen lanes own the p[j] of a frame (adjacent lanes read adjacent samples), and the tree runs as an xor butterfly over
// them; f32 addition is commutative, so every lane of the sixteen ends with the same bits and lane 0 stores them.  Neither
// the tile, the grid, the other signals nor the offset enter: a signal's values are bit-identical alone, batched and at any
// offset.  A NaN sample makes |y| NaN and with it every sum it enters: its frame, and no other.
#include <math.h>

#include "wm_internal.h"

namespace {
constexpr int CA_THREADS = 256;
constexpr int CA_LANES = 16;                                  // lanes per frame
constexpr int CA_PASS = CA_THREADS / CA_LANES;                // 16 frames per pass of the workgroup
constexpr int CA_TILE = WM_CHANACT_TILE;                      // frames per workgroup
constexpr int CA_HOP = WM_ACTIVITY_HOP;
static_assert(CA_TILE % CA_PASS == 0 && CA_HOP % CA_LANES == 0, "whole passes, whole strides");

struct CaSig {
    long long in;    // first sample of the signal
    long long n;     // samples
    long long out;   // first value of the signal (packed)
};
static_assert(sizeof(CaSig) == 24, "CaSig is copied to the device as is");

struct CaBlk {
    int sig;
    int pad;
    long long f0;   // first frame of the tile
};

// One workgroup per (signal, tile of CA_TILE consecutive frames); sixteen lanes per frame, CA_TILE / 16 passes.
__global__ __launch_bounds__(CA_THREADS) void channel_activity_kernel(const float *__restrict__ pcm, const CaSig *__restrict__ sigs,
                                                                      const CaBlk *__restrict__ blks, float *__restrict__ act) {
    const CaBlk b = blks[blockIdx.x];
    const CaSig sg = sigs[b.sig];
    const int j = threadIdx.x & (CA_LANES - 1);
    const long long n_frames = (sg.n + CA_HOP - 1) / CA_HOP;
    for (int pass = 0; pass < CA_TILE / CA_PASS; ++pass) {
        const long long f = b.f0 + pass * CA_PASS + (threadIdx.x / CA_LANES);
        // (no early exit: the butterfly below needs all sixteen lanes of a frame, and they leave together -- f is theirs alike)
        if (f >= n_frames) continue;
        const long long k0 = f * CA_HOP + j;
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < CA_HOP / CA_LANES; ++i) {
            const long long k = k0 + i * CA_LANES;
            p += k < sg.n ? fabsf(pcm[sg.in + k]) : 0.f;
        }
        p += __shfl_xor(p, 8, CA_LANES);
        p += __shfl_xor(p, 4, CA_LANES);
        p += __shfl_xor(p, 2, CA_LANES);
        p += __shfl_xor(p, 1, CA_LANES);
        if (j == 0) act[sg.out + f] = p;
    }
}
}  // namespace

void wm_chanact_destroy(WmChanAct *ca) {
    if (ca->tab) (void)hipFree(ca->tab);
    *ca = WmChanAct();
}

int wm_chanact_run(WmChanAct *ca, WmProfiler *prof, hipStream_t stream, const float *d_pcm, const int64_t *offs, int S, float *d_act) {
    WM_REQUIRE(S >= 0 && S <= 65535, WM_ERR_INVALID, "channel_activity: S must be 0 .. 65535, got %d", S);
    if (S == 0) return WM_OK;
    WM_REQUIRE(offs, WM_ERR_INVALID, "channel_activity: null sample_offsets");
    std::vector<CaSig> sig(S);
    std::vector<CaBlk> blk;
    long long out = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t n = offs[s + 1] - offs[s];
        WM_REQUIRE(offs[s] >= 0 && n >= 0, WM_ERR_INVALID, "channel_activity: signal %d: offsets [%lld, %lld) invalid", s,
                   (long long)offs[s], (long long)offs[s + 1]);
        WM_REQUIRE(n <= (int64_t)1 << 40, WM_ERR_INVALID, "channel_activity: signal %d: %lld samples (0 .. 2^40)", s, (long long)n);
        const long long frames = (n + CA_HOP - 1) / CA_HOP;
        sig[s] = CaSig{offs[s], n, out};
        out += frames;
        for (long long f0 = 0; f0 < frames; f0 += CA_TILE) blk.push_back(CaBlk{s, 0, f0});
        WM_REQUIRE(blk.size() < ((size_t)1 << 24), WM_ERR_INVALID, "channel_activity: more than 2^24 - 1 tiles of %d frames in one call",
                   CA_TILE);
    }
    if (blk.empty()) return WM_OK;
    WM_REQUIRE(d_pcm && d_act, WM_ERR_INVALID, "channel_activity: null pcm16k / act_out");
    const size_t sig_b = (sizeof(CaSig) * S + 255) & ~(size_t)255, bytes = sig_b + sizeof(CaBlk) * blk.size();
    if (ca->tab_bytes < bytes) {
        WM_HIP(hipStreamSynchronize(stream));
        if (ca->tab) WM_HIP(hipFree(ca->tab));
        ca->tab = nullptr;
        ca->tab_bytes = 0;
        WM_HIP(hipMalloc(&ca->tab, bytes));
        ca->tab_bytes = bytes;
    }
    const CaSig *d_sig = (const CaSig *)ca->tab;
    const CaBlk *d_blk = (const CaBlk *)((char *)ca->tab + sig_b);
    WM_HIP(hipMemcpyAsync(ca->tab, sig.data(), sizeof(CaSig) * S, hipMemcpyHostToDevice, stream));
    WM_HIP(hipMemcpyAsync((void *)d_blk, blk.data(), sizeof(CaBlk) * blk.size(), hipMemcpyHostToDevice, stream));
    {
        WmProfScope ps(prof, "channel_activity", stream);
        channel_activity_kernel<<<(unsigned)blk.size(), CA_THREADS, 0, stream>>>(d_pcm, d_sig, d_blk, d_act);
    }
    WM_HIP(hipGetLastError());
    // the tables are pageable host memory: the copies must have read them before they go out of scope
    WM_HIP(hipStreamSynchronize(stream));
    return WM_OK;
}
