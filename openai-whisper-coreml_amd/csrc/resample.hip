// resample.hip -- audio at any sample rate -> 16 kHz mono f32 on the device: the filter (host, f64),
// the polyphase kernel and its device-pointer core.  The C-ABI entry wm_resample_16k is in api.cpp beside wm_logmel_long,
// whose input layout this produces.  Behind it the same filter with a CHANNEL MATRIX in front (DESIGN.md section 24,
// wm_resample_16k_mix): resample_mix_kernel, one signal per (recording, matrix row).
//
// The filter.  For input rate sr: g = gcd(sr, 16000), L = 16000 / g, M = sr / g, mx = max(L, M), K = 32 mx.  The prototype
// lives at the upsampled rate, j = -K .. K:
//     c = rolloff / (2 mx),   h[j] = L 2c sinc(2c j) I0(beta sqrt(1 - (j / K)^2)) / I0(beta),   sinc(x) = sin(pi x) / (pi x)
// computed in f64 and rounded once to f32.  Output n of a recording of N frames, n < ceil(N L / M):
//     y[n] = sum_k m[k] h[n M - k L],   m the mono downmix, zero outside [0, N).
//
// The kernel reads the filter as a PHASE table [L][T4]: row p = (n M) mod L holds the taps of output n in ascending k,
//     tab[p][u] = h[j0(p) - u L]  (0 where that is below -K),  j0(p) = the largest j <= K with j = p (mod L),
// so that y[n] = sum_u m[kf(n) + u] tab[p][u], kf(n) = ceil((n M - K) / L), u = 0 .. T4 - 1, T4 = the taps per output
// ceil((2K + 1) / L) rounded up to a multiple of 4.  The sum runs in ascending u through ONE f32 fma chain per output: its
// order is a function of (rate, n) alone, never of the tile, the lane or the grid -- a recording's output is bit-identical
// alone, among others and at any offset.
#include <math.h>
#include <string.h>

#include <numeric>

#include "wm_internal.h"

namespace {
constexpr int RS_THREADS = 256;
constexpr int RS_PER_LANE = 4;
constexpr int RS_TILE = RS_THREADS * RS_PER_LANE;   // outputs per workgroup

double bessel_i0(double x) {   // power series: every term positive, converges for all x (x <= 9.62 here)
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

__host__ __device__ inline long long ceil_div_ll(long long a, long long b) {   // b > 0, any a
    return a >= 0 ? (a + b - 1) / b : -((-a) / b);
}

struct RsRec {
    long long in;      // first ELEMENT of the recording in pcm (frame k, channel c: in + k C + c)
    long long out;     // first output sample
    long long n;       // input frames
    long long n_out;   // ceil(n L / M)
    const float *tab;  // phase table [L][T4]; null: the 16 kHz bypass
    int C, L, M, K, T4;
    int pad;
};
static_assert(sizeof(RsRec) == 64, "RsRec is copied to the device as is");

struct RsBlk {
    int rec;
    int pad;
    long long n0;   // first output of the tile
};

// frame k of the recording as mono f32: the f32 sum of its channels in channel order, times (float)(1.0 / C); one channel:
// the sample itself.  int16 samples are s / 32768 (exact in f32).
template <typename S>
__device__ inline float rs_sample(const S *p) {
    if constexpr (sizeof(S) == 2) return (float)(*p) * (1.0f / 32768.0f);
    else return *p;
}
template <typename S>
__device__ inline float rs_mono(const S *pcm, long long elem, int C, float inv_c) {
    const S *p = pcm + elem;
    if (C == 1) return rs_sample(p);
    float s = rs_sample(p);
    for (int c = 1; c < C; ++c) s += rs_sample(p + c);
    return s * inv_c;
}

// The tile's outputs from the staged span.  UNIFORM (L == 1): every output reads phase row 0 -- a wave-uniform address.
template <bool UNIFORM>
__device__ inline void rs_filter_tile(const RsRec &rc, long long n0, long long k_base, const float *lds, float *out) {
    float acc[RS_PER_LANE];
    int s_off[RS_PER_LANE];
    const float4 *row[RS_PER_LANE];
#pragma unroll
    for (int i = 0; i < RS_PER_LANE; ++i) {
        // (lanes past the recording's end compute a tile-mate's position: inside the staged span, never stored)
        const long long n = n0 + threadIdx.x + i * RS_THREADS;
        const long long t = n * rc.M;
        const long long kf = ceil_div_ll(t - rc.K, rc.L);
        s_off[i] = (int)(kf - k_base);
        row[i] = (const float4 *)(rc.tab + (UNIFORM ? 0 : (size_t)(t % rc.L) * rc.T4));
        acc[i] = 0.f;
    }
    const int n4 = rc.T4 >> 2;
    for (int u = 0; u < n4; ++u) {
#pragma unroll
        for (int i = 0; i < RS_PER_LANE; ++i) {
            const float4 c = row[i][u];
            const float *s = lds + s_off[i] + 4 * u;
            acc[i] = fmaf(s[0], c.x, acc[i]);
            acc[i] = fmaf(s[1], c.y, acc[i]);
            acc[i] = fmaf(s[2], c.z, acc[i]);
            acc[i] = fmaf(s[3], c.w, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < RS_PER_LANE; ++i) {
        const long long n = n0 + threadIdx.x + i * RS_THREADS;
        if (n < rc.n_out) out[rc.out + n] = acc[i];
    }
}

// One workgroup per (recording, tile of RS_TILE consecutive outputs).  The tile's input span [kf(n0), kf(n0 + RS_TILE - 1)
// + T4) is downmixed into LDS once, zeros outside the recording; then every lane runs the fma chains of its outputs
// n0 + lane + 256 i (adjacent lanes read LDS words M / L apart).
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const S *__restrict__ pcm, const RsRec *__restrict__ recs,
                                                              const RsBlk *__restrict__ blks, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const RsBlk b = blks[blockIdx.x];
    const RsRec rc = recs[b.rec];
    const float inv_c = (float)(1.0 / (double)rc.C);
    if (rc.tab == nullptr) {   // 16 kHz: the downmix alone
#pragma unroll
        for (int i = 0; i < RS_PER_LANE; ++i) {
            const long long n = b.n0 + threadIdx.x + i * RS_THREADS;
            if (n < rc.n_out) out[rc.out + n] = rs_mono(pcm, rc.in + n * rc.C, rc.C, inv_c);
        }
        return;
    }
    const long long k_base = ceil_div_ll(b.n0 * rc.M - rc.K, rc.L);
    const long long k_last = ceil_div_ll((b.n0 + RS_TILE - 1) * rc.M - rc.K, rc.L);
    const int span = (int)(k_last - k_base) + rc.T4;
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long k = k_base + i;
        rs_lds[i] = (k >= 0 && k < rc.n) ? rs_mono(pcm, rc.in + k * rc.C, rc.C, inv_c) : 0.f;
    }
    __syncthreads();
    if (rc.L == 1) rs_filter_tile<true>(rc, b.n0, k_base, rs_lds, out);
    else rs_filter_tile<false>(rc, b.n0, k_base, rs_lds, out);
}

// ---- the channel matrix (wm_resample_16k_mix) ----
// One output signal: a recording's geometry (out: the SIGNAL's first output sample) and its row of weights.
struct RsSig {
    RsRec rc;
    float w[WM_RS_MAX_CHANNELS];
};
static_assert(sizeof(RsSig) == 96, "RsSig is copied to the device as is");

// frame k under a row w: m = w[0] x[0] (one rounding), then m = fmaf(w[c], x[c], m) in channel order
template <typename S>
__device__ inline float rs_mix(const S *pcm, long long elem, int C, const float *w) {
    const S *p = pcm + elem;
    float m = w[0] * rs_sample(p);
    for (int c = 1; c < C; ++c) m = fmaf(w[c], rs_sample(p + c), m);
    return m;
}

// resample_kernel with the row's mix where the mean was: one workgroup per (signal, tile of RS_TILE outputs), each re-reading
// the interleaved span of its tile.  The staged span and the fma chains are resample_kernel's, so a signal's bits are a
// function of (recording, rate, row) alone.
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void resample_mix_kernel(const S *__restrict__ pcm, const RsSig *__restrict__ sigs,
                                                                  const RsBlk *__restrict__ blks, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const RsBlk b = blks[blockIdx.x];
    const RsRec rc = sigs[b.rec].rc;
    const float *w = sigs[b.rec].w;   // (a wave-uniform address: the weights come through the scalar cache)
    if (rc.tab == nullptr) {   // 16 kHz: the mix alone
#pragma unroll
        for (int i = 0; i < RS_PER_LANE; ++i) {
            const long long n = b.n0 + threadIdx.x + i * RS_THREADS;
            if (n < rc.n_out) out[rc.out + n] = rs_mix(pcm, rc.in + n * rc.C, rc.C, w);
        }
        return;
    }
    const long long k_base = ceil_div_ll(b.n0 * rc.M - rc.K, rc.L);
    const long long k_last = ceil_div_ll((b.n0 + RS_TILE - 1) * rc.M - rc.K, rc.L);
    const int span = (int)(k_last - k_base) + rc.T4;
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long k = k_base + i;
        rs_lds[i] = (k >= 0 && k < rc.n) ? rs_mix(pcm, rc.in + k * rc.C, rc.C, w) : 0.f;
    }
    __syncthreads();
    if (rc.L == 1) rs_filter_tile<true>(rc, b.n0, k_base, rs_lds, out);
    else rs_filter_tile<false>(rc, b.n0, k_base, rs_lds, out);
}

// floats of LDS a tile of this rate can need: (kf(n0 + RS_TILE - 1) - kf(n0)) + T4 <= ceil((RS_TILE - 1) M / L) + T4
size_t rs_span_floats(int L, int M, int T4) { return (size_t)(((long long)(RS_TILE - 1) * M + L - 1) / L) + (size_t)T4; }
}  // namespace

bool wm_resample_params(long long sample_rate, int *L, int *M, int *K) {
    if (sample_rate < WM_RS_MIN_RATE || sample_rate > WM_RS_MAX_RATE) return false;
    const int sr = (int)sample_rate, g = std::gcd(sr, WM_RS_TARGET_RATE);
    const int l = WM_RS_TARGET_RATE / g, m = sr / g;
    if (l > WM_RS_MAX_L) return false;
    *L = l;
    *M = m;
    *K = WM_RESAMPLE_ZEROS * (l > m ? l : m);
    return true;
}

void wm_resample_prototype(int L, int M, int K, std::vector<float> &h) {
    const double PI = 3.14159265358979323846264338327950288;
    const int mx = L > M ? L : M;
    const double c = WM_RESAMPLE_ROLLOFF / (2.0 * mx), i0b = bessel_i0(WM_RESAMPLE_BETA);
    h.assign((size_t)2 * K + 1, 0.f);
    for (int j = 0; j <= K; ++j) {
        const double x = 2.0 * c * j, r = (double)j / (double)K;
        const double sinc = j == 0 ? 1.0 : sin(PI * x) / (PI * x);
        const double w = bessel_i0(WM_RESAMPLE_BETA * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / i0b;
        const float v = (float)((double)L * 2.0 * c * sinc * w);
        h[(size_t)K + j] = v;   // the one rounding; the mirror makes the table symmetric bit for bit
        h[(size_t)K - j] = v;
    }
}

void wm_resample_destroy(WmResampler *rs) {
    for (auto &kv : rs->filt)
        if (kv.second.d_tab) (void)hipFree(kv.second.d_tab);
    if (rs->tab) (void)hipFree(rs->tab);
    *rs = WmResampler();
}

// the rate's phase table, built and uploaded on first use
static int rs_filter(WmResampler *rs, hipStream_t stream, int sr, const WmRsFilter **out) {
    auto it = rs->filt.find(sr);
    if (it != rs->filt.end()) {
        *out = &it->second;
        return WM_OK;
    }
    WmRsFilter f;
    WM_REQUIRE(wm_resample_params(sr, &f.L, &f.M, &f.K), WM_ERR_INVALID, "resample: unsupported sample rate %d", sr);
    std::vector<float> h;
    wm_resample_prototype(f.L, f.M, f.K, h);
    const int T = (2 * f.K + 1 + f.L - 1) / f.L;
    f.T4 = (T + 3) & ~3;
    std::vector<float> tab((size_t)f.L * f.T4, 0.f);
    for (int p = 0; p < f.L; ++p) {
        const long long j0 = p + (long long)f.L * ((f.K - p) / f.L);
        for (int u = 0; u < f.T4; ++u) {
            const long long j = j0 - (long long)u * f.L;
            if (j >= -(long long)f.K) tab[(size_t)p * f.T4 + u] = h[(size_t)(j + f.K)];
        }
    }
    WM_HIP(hipMalloc((void **)&f.d_tab, tab.size() * sizeof(float)));
    hipError_t e = hipMemcpyAsync(f.d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // `tab` is pageable and leaves scope here
    if (e != hipSuccess) {
        (void)hipFree(f.d_tab);
        wm_set_error("resample: filter upload failed: %s", hipGetErrorString(e));
        return WM_ERR_HIP;
    }
    *out = &(rs->filt[sr] = f);
    return WM_OK;
}

// Recording r's geometry (everything of RsRec but `out`) after the checks both entries share; *lds_floats grows to the span
// a tile of its rate needs.
static int rs_record(WmResampler *rs, hipStream_t stream, int r, const int64_t *offs, const int32_t *n_channels,
                     const int32_t *sample_rates, RsRec *rec, size_t *lds_floats) {
    const int64_t len = offs[r + 1] - offs[r];
    const int C = n_channels[r], sr = sample_rates[r];
    WM_REQUIRE(offs[r] >= 0 && len >= 0, WM_ERR_INVALID, "resample: recording %d: offsets [%lld, %lld) invalid", r,
               (long long)offs[r], (long long)offs[r + 1]);
    WM_REQUIRE(C >= 1 && C <= WM_RS_MAX_CHANNELS, WM_ERR_INVALID, "resample: recording %d: %d channels (1 .. %d)", r, C,
               WM_RS_MAX_CHANNELS);
    WM_REQUIRE(len % C == 0, WM_ERR_INVALID, "resample: recording %d: %lld samples are no multiple of its %d channels", r,
               (long long)len, C);
    const int64_t n_out = wm_resample_out_len(len / C, sr);
    WM_REQUIRE(n_out >= 0, WM_ERR_INVALID, "resample: recording %d: unsupported sample rate %d", r, sr);
    WM_REQUIRE(n_out <= (int64_t)1 << 30, WM_ERR_INVALID, "resample: recording %d: %lld output samples (0 .. 2^30)", r,
               (long long)n_out);
    RsRec &rc = *rec;
    rc.in = offs[r];
    rc.out = 0;
    rc.n = len / C;
    rc.n_out = n_out;
    rc.C = C;
    rc.pad = 0;
    if (sr == WM_RS_TARGET_RATE) {
        rc.tab = nullptr;
        rc.L = rc.M = 1;
        rc.K = rc.T4 = 0;
    } else {
        const WmRsFilter *f = nullptr;
        WM_TRY(rs_filter(rs, stream, sr, &f));
        rc.tab = f->d_tab;
        rc.L = f->L;
        rc.M = f->M;
        rc.K = f->K;
        rc.T4 = f->T4;
        const size_t need = rs_span_floats(f->L, f->M, f->T4);
        if (n_out > 0 && need > *lds_floats) *lds_floats = need;
    }
    return WM_OK;
}

// The call's tables on the device: rec_bytes of records (RsRec or RsSig), then the workgroup table; the copies are queued.
static int rs_tables(WmResampler *rs, hipStream_t stream, const void *rec, size_t rec_bytes, const std::vector<RsBlk> &blk,
                     const void *d_pcm, const float *d_out, size_t lds_floats, const void **d_rec, const RsBlk **d_blk) {
    // (grid limit: blocks x 256 lanes stays below 2^32 -- 2^24 - 1 tiles are 298 hours of 16 kHz output)
    WM_REQUIRE(blk.size() < ((size_t)1 << 24), WM_ERR_INVALID, "resample: %zu tiles of %d outputs in one call (at most 2^24 - 1)",
               blk.size(), RS_TILE);
    WM_REQUIRE(d_pcm && d_out, WM_ERR_INVALID, "resample: null pcm / out");
    WM_REQUIRE(lds_floats * sizeof(float) <= 64 * 1024, WM_ERR_INVALID, "resample: tile span of %zu floats", lds_floats);
    const size_t rec_b = (rec_bytes + 255) & ~(size_t)255, bytes = rec_b + sizeof(RsBlk) * blk.size();
    if (rs->tab_bytes < bytes) {
        WM_HIP(hipStreamSynchronize(stream));
        if (rs->tab) WM_HIP(hipFree(rs->tab));
        rs->tab = nullptr;
        rs->tab_bytes = 0;
        WM_HIP(hipMalloc(&rs->tab, bytes));
        rs->tab_bytes = bytes;
    }
    *d_rec = rs->tab;
    *d_blk = (const RsBlk *)((char *)rs->tab + rec_b);
    WM_HIP(hipMemcpyAsync(rs->tab, rec, rec_bytes, hipMemcpyHostToDevice, stream));
    WM_HIP(hipMemcpyAsync((void *)*d_blk, blk.data(), sizeof(RsBlk) * blk.size(), hipMemcpyHostToDevice, stream));
    return WM_OK;
}

int wm_resample_run(WmResampler *rs, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype,
                    const int64_t *offs, const int32_t *n_channels, const int32_t *sample_rates, int R, float *d_out) {
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32, WM_ERR_INVALID, "resample: pcm dtype must be WM_I16 / WM_F32");
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "resample: R must be 0 .. 65535, got %d", R);
    if (R == 0) return WM_OK;
    WM_REQUIRE(offs && n_channels && sample_rates, WM_ERR_INVALID, "resample: null offsets / n_channels / sample_rates");
    std::vector<RsRec> rec(R);
    std::vector<RsBlk> blk;
    long long out = 0;
    size_t lds_floats = 0;
    for (int r = 0; r < R; ++r) {
        WM_TRY(rs_record(rs, stream, r, offs, n_channels, sample_rates, &rec[r], &lds_floats));
        rec[r].out = out;
        out += rec[r].n_out;
        for (long long n0 = 0; n0 < rec[r].n_out; n0 += RS_TILE) blk.push_back(RsBlk{r, 0, n0});
    }
    if (blk.empty()) return WM_OK;
    const void *d_tab = nullptr;
    const RsBlk *d_blk = nullptr;
    WM_TRY(rs_tables(rs, stream, rec.data(), sizeof(RsRec) * R, blk, d_pcm, d_out, lds_floats, &d_tab, &d_blk));
    const RsRec *d_rec = (const RsRec *)d_tab;
    {
        WmProfScope ps(prof, "resample", stream);
        const size_t lds = lds_floats * sizeof(float);
        if (pcm_dtype == WM_I16)
            resample_kernel<int16_t><<<(unsigned)blk.size(), RS_THREADS, lds, stream>>>((const int16_t *)d_pcm, d_rec, d_blk, d_out);
        else
            resample_kernel<float><<<(unsigned)blk.size(), RS_THREADS, lds, stream>>>((const float *)d_pcm, d_rec, d_blk, d_out);
    }
    WM_HIP(hipGetLastError());
    // the tables are pageable host memory: the copies must have read them before they go out of scope
    WM_HIP(hipStreamSynchronize(stream));
    return WM_OK;
}

int wm_resample_mix_run(WmResampler *rs, WmProfiler *prof, hipStream_t stream, const void *d_pcm, wm_dtype pcm_dtype,
                        const int64_t *offs, const int32_t *n_channels, const int32_t *sample_rates, int R, const int32_t *n_rows,
                        const float *mix, float *d_out) {
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32, WM_ERR_INVALID, "resample: pcm dtype must be WM_I16 / WM_F32");
    WM_REQUIRE(R >= 0 && R <= 65535, WM_ERR_INVALID, "resample: R must be 0 .. 65535, got %d", R);
    if (R == 0) return WM_OK;
    WM_REQUIRE(offs && n_channels && sample_rates, WM_ERR_INVALID, "resample: null offsets / n_channels / sample_rates");
    WM_REQUIRE(n_rows && mix, WM_ERR_INVALID, "resample_mix: null n_rows / mix");
    std::vector<RsSig> sig;
    std::vector<RsBlk> blk;
    long long out = 0;
    size_t lds_floats = 0;
    const float *w = mix;
    for (int r = 0; r < R; ++r) {
        RsSig s;
        WM_TRY(rs_record(rs, stream, r, offs, n_channels, sample_rates, &s.rc, &lds_floats));
        WM_REQUIRE(n_rows[r] >= 1 && n_rows[r] <= WM_RS_MAX_CHANNELS, WM_ERR_INVALID, "resample_mix: recording %d: %d rows (1 .. %d)",
                   r, n_rows[r], WM_RS_MAX_CHANNELS);
        WM_REQUIRE(sig.size() + (size_t)n_rows[r] <= 65535, WM_ERR_INVALID, "resample_mix: more than 65535 output signals");
        for (int o = 0; o < n_rows[r]; ++o, w += s.rc.C) {
            for (int c = 0; c < WM_RS_MAX_CHANNELS; ++c) s.w[c] = c < s.rc.C ? w[c] : 0.f;
            for (int c = 0; c < s.rc.C; ++c)
                WM_REQUIRE(std::isfinite(w[c]), WM_ERR_INVALID, "resample_mix: recording %d, row %d: weight %d is not finite", r, o, c);
            s.rc.out = out;
            out += s.rc.n_out;
            for (long long n0 = 0; n0 < s.rc.n_out; n0 += RS_TILE) blk.push_back(RsBlk{(int)sig.size(), 0, n0});
            sig.push_back(s);
        }
    }
    if (blk.empty()) return WM_OK;
    const void *d_tab = nullptr;
    const RsBlk *d_blk = nullptr;
    WM_TRY(rs_tables(rs, stream, sig.data(), sizeof(RsSig) * sig.size(), blk, d_pcm, d_out, lds_floats, &d_tab, &d_blk));
    const RsSig *d_sig = (const RsSig *)d_tab;
    {
        WmProfScope ps(prof, "resample_mix", stream);
        const size_t lds = lds_floats * sizeof(float);
        if (pcm_dtype == WM_I16)
            resample_mix_kernel<int16_t><<<(unsigned)blk.size(), RS_THREADS, lds, stream>>>((const int16_t *)d_pcm, d_sig, d_blk, d_out);
        else
            resample_mix_kernel<float><<<(unsigned)blk.size(), RS_THREADS, lds, stream>>>((const float *)d_pcm, d_sig, d_blk, d_out);
    }
    WM_HIP(hipGetLastError());
    // the tables are pageable host memory: the copies must have read them before they go out of scope
    WM_HIP(hipStreamSynchronize(stream));
    return WM_OK;
}

extern "C" int64_t wm_resample_out_len(int64_t n_frames, int sample_rate) {
    int L, M, K;
    if (n_frames < 0 || n_frames > ((int64_t)1 << 40) || !wm_resample_params(sample_rate, &L, &M, &K)) return -1;
    return (n_frames * L + M - 1) / M;
}

extern "C" int wm_resample_filter(int sample_rate, float *h, size_t cap, int *L, int *M, int *K) try {
    int l, m, k;
    WM_REQUIRE(wm_resample_params(sample_rate, &l, &m, &k), WM_ERR_INVALID,
               "resample: unsupported sample rate %d (%d .. %d Hz with 16000 / gcd(rate, 16000) <= %d)", sample_rate,
               WM_RS_MIN_RATE, WM_RS_MAX_RATE, WM_RS_MAX_L);
    if (L) *L = l;
    if (M) *M = m;
    if (K) *K = k;
    if (cap == 0) return WM_OK;   // sizing call: the table has 2 K + 1 entries
    WM_REQUIRE(h && cap >= (size_t)2 * k + 1, WM_ERR_INVALID, "resample_filter: the table needs %d floats, cap is %zu", 2 * k + 1, cap);
    std::vector<float> tab;
    wm_resample_prototype(l, m, k, tab);
    memcpy(h, tab.data(), tab.size() * sizeof(float));
    return WM_OK;
} WM_API_CATCH
