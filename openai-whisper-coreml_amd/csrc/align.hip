// align.hip -- word-level timestamps on the GPU (wm_align): openai-whisper's find_alignment (whisper/timing.py) after the
// teacher-forced decoder pass.
//
//   * align_capture_kernel: inside the teacher-forced pass, the alignment heads' 64-wide cross-attention queries of the
//     current decode position (read from HBM: the device-side position) -> the capture buffer q [B][T][J][64] f32.
//     An aligned transcribe group (wm_transcribe_mel_aligned) captures inside its OWN decode steps, eager or replayed from the
//     position graphs: the <false, true> instantiation writes capture row position - base, base = the group's
//     <|startoftranscript|> position, and nothing in front of it.
//   * align_gather_kernel: an aligned best-of / beam group (wm_transcribe_mel_beam_aligned) captures every row of a window; the
//     rows of the ONE hypothesis that is aligned are copied, capture row by capture row from the slot that held them
//     (wm_beam_ancestry), into a buffer laid out as a plain aligned group's -- 16-byte vector copies, no LDS.
//   * align_token_prob_kernel: softmax(logits[S + i][0 : eot])[t[i]] per chunk, from the logits row of the position.
//   * align_stats_kernel (pass 1, one workgroup per (chunk, head)): the scores q.k / 8 * qk_scale over frames [0, M) are
//     recomputed from the bf16 cross-K cache with the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain),
//     16 decoder rows x 16 frames per tile.  Sweep 1 gives every row its softmax (max, 1 / sum); sweep 2 the per-frame sums
//     of p over the chunk's rows, hence the column means; sweep 3 the per-frame sums of (p - mean)^2, hence the stds (two
//     passes: the one-pass E[p^2] - mean^2 cancels to nothing in f32 once std / mean falls to ~1e-3).  Each wave owns its LDS
//     column partials, summed in wave order: no float atomics.
//     Out: row statistics [B][J][T][2] and column (mean, std) [B][J][1500][2] -- never the [J][T][1500] probabilities.
//     The row rule (WmAlignDev::tail, n_min): a chunk has T = S + n + 1 + tail decoder rows, of which rows S .. S + n are the cost
//     matrix.  wm_align: tail 1 (the teacher-forced eot's row), a chunk needs n >= 1.  An aligned transcribe group: tail 0 (a
//     decode never feeds its last token), n = len - 1 >= 0, absent rows -1.  Rows at or past T of the capture buffer -- where a
//     stopped row of a decode group keeps writing -- are never read: every row index is clamped to T - 1.
//   * align_matrix_kernel (pass 2, one workgroup per (chunk, 16 text rows, 64 frames)): for every head in ascending
//     (layer, head) order it recomputes the scores of its rows over its frames plus the filter's halo, normalises them
//     (softmax, z-score), applies the median filter (reflect padding) and adds the result to a register accumulator; the
//     cost matrix is x = -(sum / J).  One thread owns each output cell for the whole head loop: a fixed summation order.
//   * dtw_kernel (one wave per chunk): dynamic time warping over the anti-diagonals k = i + j, the last three diagonals of
//     costs in LDS, the 2-bit trace packed per row in registers and stored a word (16 cells) at a time -- into LDS when the
//     chunk's trace fits (typical: 225 rows x 94 words = 84.6 KB), else into HBM -- then the backtrace of lane 0.
#include "dtw.h"
#include "model.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int AL_OUT = 64;        // output frames per workgroup of the matrix kernel
constexpr int AL_MAXHALF = 15;    // medfilt_width <= 31
constexpr int AL_ZW = AL_OUT + 2 * AL_MAXHALF + 2;   // LDS row of one head's normalised scores (frames + halo)
constexpr int AL_MAXT = 448;      // decoder rows S + n + 2 <= n_text_ctx <= 448
constexpr int DTW_ROWS_PER_LANE = (AL_MAXT + 63) / 64;   // text rows <= n_text_ctx

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// q of the lane's query row, elements 16 g .. 16 g + 15 (g = lane >> 4)
__device__ __forceinline__ void load_q(const float *p, float qf[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = ((const float4 *)p)[i];
        qf[4 * i] = v.x; qf[4 * i + 1] = v.y; qf[4 * i + 2] = v.z; qf[4 * i + 3] = v.w;
    }
}

// 16 query rows x 16 frames of q.k.  Lane l supplies A[row l & 15][k = l >> 4] = q[row][16 (l >> 4) + s] and
// B[k = l >> 4][col l & 15] = k[frame][16 (l >> 4) + s] at step s; it gets D[row 4 (l >> 4) + r][col l & 15] in acc[r].
__device__ __forceinline__ f32x4 score_tile(const float qf[16], const bf16_t *krow) {
    const uint4 a = ((const uint4 *)krow)[0], b = ((const uint4 *)krow)[1];
    const float kf[16] = {bf_lo(a.x), bf_hi(a.x), bf_lo(a.y), bf_hi(a.y), bf_lo(a.z), bf_hi(a.z), bf_lo(a.w), bf_hi(a.w),
                          bf_lo(b.x), bf_hi(b.x), bf_lo(b.y), bf_hi(b.y), bf_lo(b.z), bf_hi(b.z), bf_lo(b.w), bf_hi(b.w)};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[s], kf[s], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ const bf16_t *head_keys(const WmAlignDev &a, int b, int j) {
    return a.xkv + ((size_t)(a.hl[j] * 2 * a.B + b) * a.H + a.hh[j]) * 1500 * 64;
}
__device__ __forceinline__ const float *head_query(const WmAlignDev &a, int b, int t, int j) {
    return a.q + (((size_t)b * a.Tq + t) * a.J + j) * 64;
}

// (max, sum) pairs of a softmax in log2 units
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    s = (m == mm ? s : s * exp2f(m - mm)) + (m2 == mm ? s2 : s2 * exp2f(m2 - mm));
    m = mm;
}

// PANEL (a teacher-forced panel step, wm_set_teacher_panel): dq row r is position *pos_ptr + r % w of chunk r / w; the capture
// layout is unchanged.  Instantiations of their own, here and in the token-probability kernel: the step kernels stay as they were.
// BASED (an aligned transcribe group, its own instantiation too): w is the absolute position of capture row 0 -- the group's
// <|startoftranscript|> position --, the positions in front of it are not captured.  A row that has stopped keeps writing its
// (stale) query at the group's position: rows past a chunk's own T, which the alignment kernels clamp away.
template <bool PANEL, bool BASED = false>
__global__ __launch_bounds__(64) void align_capture_kernel(const float *__restrict__ dq, int d, const int *__restrict__ pos_ptr,
                                                           WmAlignLayer L, float *__restrict__ cap, int Tq, int J, int w) {
    const int r = blockIdx.x, k = blockIdx.y;
    int b = r, pos = *pos_ptr;
    if constexpr (PANEL) {
        b = r / w;
        pos += r - b * w;
    }
    if constexpr (BASED) {
        pos -= w;
        if (pos < 0) return;
    }
    if (pos >= Tq) return;
    cap[(((size_t)b * Tq + pos) * J + L.slot0 + k) * 64 + threadIdx.x] = dq[(size_t)r * d + L.head[k] * 64 + threadIdx.x];
}

// The chosen hypothesis' queries of an aligned best-of / beam group (wm_align_gather): grid (tile of AL_GATHER_ROWS capture rows,
// window).  Capture row t of window c is J * 256 contiguous bytes in row c * N + slot[c][t] of the capture buffer and goes to
// row c of q_sel: consecutive lanes move consecutive 16-byte units, a wave 1 KiB per instruction.  Rows at or past n_rows[c]
// are not touched.
constexpr int AL_GATHER_ROWS = 4;
__global__ __launch_bounds__(256) void align_gather_kernel(const uint4 *__restrict__ cap, uint4 *__restrict__ q_sel,
                                                           const int *__restrict__ slot, const int *__restrict__ n_rows, int N, int Tq,
                                                           int J) {
    const int c = blockIdx.y, R = min(n_rows[c], Tq);
    const size_t row_u = (size_t)J * 16;   // 16-byte units of one capture row
    for (int t = blockIdx.x * AL_GATHER_ROWS; t < (blockIdx.x + 1) * AL_GATHER_ROWS && t < R; ++t) {
        const int s = min(max(slot[(size_t)c * Tq + t], 0), N - 1);
        const uint4 *src = cap + (((size_t)c * N + s) * Tq + t) * row_u;
        uint4 *dst = q_sel + ((size_t)c * Tq + t) * row_u;
        for (size_t u = threadIdx.x; u < row_u; u += 256) dst[u] = src[u];
    }
}

// B: chunks per position of seq.  PANEL: logits row r is position *pos_ptr + r % w of chunk r / w, and the row takes a
// probability only when ITS position is one of the chunk's text positions.
template <bool PANEL>
__global__ __launch_bounds__(256) void align_token_prob_kernel(const float *__restrict__ logits, long ldo,
                                                               const int *__restrict__ seq, const int *__restrict__ pos_ptr,
                                                               int B, int S, int eot, const int *__restrict__ n_text,
                                                               float *__restrict__ prob, int max_text, int w) {
    __shared__ float red[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    int b = r, pos = *pos_ptr;
    if constexpr (PANEL) {
        b = r / w;
        pos += r - b * w;
    }
    const int i = pos - S;
    if (i < 0 || i >= n_text[b]) return;
    const float *row = logits + (long)r * ldo;
    float m = -INFINITY;
    for (int v = tid; v < eot; v += 256) m = fmaxf(m, row[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int v = tid; v < eot; v += 256) s += expf(row[v] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const int tok = seq[(long)(pos + 1) * B + b];
        prob[(long)b * max_text + i] = expf(row[tok] - m) / ((red[0] + red[1]) + (red[2] + red[3]));
    }
}

__global__ __launch_bounds__(256) void align_stats_kernel(WmAlignDev a) {
    __shared__ float part[4][1500];      // per-wave column sums: of p (sweep 2), then of (p - mean)^2 (sweep 3)
    __shared__ float mean[1500];
    __shared__ float rowl[AL_MAXT][2];   // the rows' (max, 1 / sum) for sweep 3
    const int j = blockIdx.x, b = blockIdx.y, n = a.n_text[b];
    if (n < a.n_min) return;
    const int T = a.S + n + 1 + a.tail, M = a.n_frames[b] / 2;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    for (int i = threadIdx.x; i < 4 * 1500; i += 256) (&part[0][0])[i] = 0.f;
    __syncthreads();
    const bf16_t *K = head_keys(a, b, j);
    const int nft = (M + 15) / 16;
    for (int t0 = w * 16; t0 < T; t0 += 64) {
        float qf[16];
        load_q(head_query(a, b, min(t0 + c, T - 1), j) + 16 * g, qf);
        float m[4], s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; s[r] = 0.f; }
        for (int ft = 0; ft < nft; ++ft) {
            const int f = ft * 16 + c;
            const f32x4 acc = score_tile(qf, K + (size_t)min(f, M - 1) * 64 + 16 * g);
            if (f < M) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[r] * a.sc;
                    if (v > m[r]) { s[r] = s[r] * exp2f(m[r] - v) + 1.f; m[r] = v; }
                    else s[r] += exp2f(v - m[r]);
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
            for (int r = 0; r < 4; ++r) lse_merge(m[r], s[r], __shfl_xor(m[r], o), __shfl_xor(s[r], o));
        float inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            inv[r] = 1.f / s[r];
            const int t = t0 + 4 * g + r;
            if (c == 0 && t < T) {
                float *rs = a.rowst + (((size_t)b * a.J + j) * a.Tq + t) * 2;
                rs[0] = rowl[t][0] = m[r];
                rs[1] = rowl[t][1] = inv[r];
            }
        }
        for (int ft = 0; ft < nft; ++ft) {
            const int f = ft * 16 + c;
            const f32x4 acc = score_tile(qf, K + (size_t)min(f, M - 1) * 64 + 16 * g);
            float p1 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (f < M && t0 + 4 * g + r < T) p1 += exp2f(acc[r] * a.sc - m[r]) * inv[r];
            p1 += __shfl_xor(p1, 16);
            p1 += __shfl_xor(p1, 32);
            if (g == 0 && f < M) part[w][f] += p1;
        }
    }
    __syncthreads();
    const float inv_T = 1.f / (float)T;
    for (int f = threadIdx.x; f < M; f += 256) {   // one thread per frame: reads its partials, then clears them
        mean[f] = (((part[0][f] + part[1][f]) + part[2][f]) + part[3][f]) * inv_T;
        part[0][f] = part[1][f] = part[2][f] = part[3][f] = 0.f;
    }
    __syncthreads();
    for (int t0 = w * 16; t0 < T; t0 += 64) {   // sweep 3: the same p once more, its squared deviation from the column mean
        float qf[16];
        load_q(head_query(a, b, min(t0 + c, T - 1), j) + 16 * g, qf);
        float m[4], inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = min(t0 + 4 * g + r, T - 1);
            m[r] = rowl[t][0];
            inv[r] = rowl[t][1];
        }
        for (int ft = 0; ft < nft; ++ft) {
            const int f = ft * 16 + c;
            const f32x4 acc = score_tile(qf, K + (size_t)min(f, M - 1) * 64 + 16 * g);
            float d2 = 0.f;
            if (f < M) {
                const float mu = mean[f];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t0 + 4 * g + r < T) {
                        const float d = exp2f(acc[r] * a.sc - m[r]) * inv[r] - mu;
                        d2 += d * d;
                    }
            }
            d2 += __shfl_xor(d2, 16);
            d2 += __shfl_xor(d2, 32);
            if (g == 0 && f < M) part[w][f] += d2;
        }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < M; f += 256) {
        const float s2 = ((part[0][f] + part[1][f]) + part[2][f]) + part[3][f];
        float *cs = a.colst + (((size_t)b * a.J + j) * 1500 + f) * 2;
        cs[0] = mean[f];
        cs[1] = sqrtf(s2 * inv_T);
    }
}

// torch F.pad(mode="reflect") index of frame ff of a row of M frames (|ff| < M)
__device__ __forceinline__ int reflect(int ff, int M) {
    ff = ff < 0 ? -ff : ff;
    return ff >= M ? 2 * (M - 1) - ff : ff;
}

// torch's sort-based median of the 2h + 1 values around frame fo (reflect padding), as the value of stable rank h
template <int WMAX>
__device__ __forceinline__ float median_reflect(const float *zrow, int fo, int h, int lo, int M) {
    const int w = 2 * h + 1;
    float v[WMAX];
#pragma unroll
    for (int u = 0; u < WMAX; ++u) {
        v[u] = u < w ? zrow[reflect(fo - h + u, M) - lo] : 0.f;
    }
    float med = v[0];
#pragma unroll
    for (int u = 0; u < WMAX; ++u) {
        int cnt = 0;
#pragma unroll
        for (int u2 = 0; u2 < WMAX; ++u2) cnt += (u2 < w) && (v[u2] < v[u] || (v[u2] == v[u] && u2 < u));
        if (u < w && cnt == h) med = v[u];
    }
    return med;
}

// wider windows (up to 31): the same rule with the values read from LDS (no register array to spill)
__device__ float median_reflect_lds(const float *zrow, int fo, int h, int lo, int M) {
    const int w = 2 * h + 1;
    float med = 0.f;
    for (int u = 0; u < w; ++u) {
        const float vu = zrow[reflect(fo - h + u, M) - lo];
        int cnt = 0;
        for (int u2 = 0; u2 < w; ++u2) {
            const float v2 = zrow[reflect(fo - h + u2, M) - lo];
            cnt += v2 < vu || (v2 == vu && u2 < u);
        }
        if (cnt == h) med = vu;
    }
    return med;
}

// WMAX = 7: windows up to 7 from registers; WMAX = 0: any window up to 31 from LDS
template <int WMAX>
__global__ __launch_bounds__(256) void align_matrix_kernel(WmAlignDev a) {
    __shared__ float zl[16][AL_ZW];
    const int b = blockIdx.z, n = a.n_text[b];
    const int N = n + 1, i0 = blockIdx.y * 16, f0 = blockIdx.x * AL_OUT, M = a.n_frames[b] / 2;
    if (n < a.n_min || i0 >= N || f0 >= M) return;
    const int T = a.S + n + 1 + a.tail, h = a.half;
    const bool filt = h > 0 && M > h;   // openai-whisper: no filtering when the window's padding would not fit
    const int lo = filt ? max(0, f0 - h) : f0, hi = filt ? min(M, f0 + AL_OUT + h) : min(M, f0 + AL_OUT);
    const int ntile = (hi - lo + 15) / 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int ro = threadIdx.x >> 4;    // the output row of this thread; its frames: f0 + (tid & 15) + 16 k
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.J; ++j) {
        const bf16_t *K = head_keys(a, b, j);
        if (w < ntile) {
            float qf[16];
            load_q(head_query(a, b, min(a.S + i0 + c, T - 1), j) + 16 * g, qf);
            for (int tt = w; tt < ntile; tt += 4) {
                const int f = lo + tt * 16 + c;
                const f32x4 sc = score_tile(qf, K + (size_t)min(f, M - 1) * 64 + 16 * g);
                if (f < hi) {
                    const float *cs = a.colst + (((size_t)b * a.J + j) * 1500 + f) * 2;
                    const float mean = cs[0], sd = cs[1];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = i0 + 4 * g + r;
                        float z = 0.f;
                        if (i < N) {
                            const float *rs = a.rowst + (((size_t)b * a.J + j) * a.Tq + a.S + i) * 2;
                            const float p = exp2f(sc[r] * a.sc - rs[0]) * rs[1];
                            z = (p - mean) / sd;
                        }
                        zl[4 * g + r][f - lo] = z;
                    }
                }
            }
        }
        __syncthreads();
        if (i0 + ro < N) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int fo = f0 + (threadIdx.x & 15) + 16 * k;
                if (fo < min(M, f0 + AL_OUT))
                    acc[k] += !filt ? zl[ro][fo - lo]
                              : WMAX > 0 ? median_reflect<(WMAX > 0 ? WMAX : 1)>(zl[ro], fo, h, lo, M)
                                         : median_reflect_lds(zl[ro], fo, h, lo, M);
            }
        }
        __syncthreads();
    }
    if (i0 + ro < N) {
        float *xr = a.x + ((size_t)b * a.n_ld + i0 + ro) * 1500;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int fo = f0 + (threadIdx.x & 15) + 16 * k;
            if (fo < min(M, f0 + AL_OUT)) xr[fo] = -(acc[k] / (float)a.J);
        }
    }
}

template <bool LDS_TRACE>
__global__ __launch_bounds__(64) void dtw_kernel(const float *__restrict__ x, long x_bstride, int ld, const int *__restrict__ Nv,
                                                 const int *__restrict__ Mv, unsigned *__restrict__ trace_g, long tr_bstride,
                                                 int *__restrict__ start, int n_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, lane = threadIdx.x, N = Nv[b], M = Mv[b];
    int *out = start + (long)b * n_out;
    for (int i = lane; i < n_out; i += 64) out[i] = -1;
    if (N <= 0 || M <= 0) return;
    const int W = (M + 15) / 16;           // trace words per row: cell (i, j) at bits 2 ((j - 1) % 16) of word (j - 1) / 16
    float *D = (float *)smem;              // [3][N + 1]: D[k % 3][i] = cost[i][k - i]
    unsigned *tr = LDS_TRACE ? (unsigned *)(D + 3 * (N + 1)) : trace_g + (long)b * tr_bstride;   // [N][W], text row i - 1
    const float *xb = x + (long)b * x_bstride;
    if (lane == 0) { D[0] = 0.f; D[N + 1] = INFINITY; D[N + 2] = INFINITY; }   // diagonals 0 and 1
    unsigned word[DTW_ROWS_PER_LANE];
    float xn[DTW_ROWS_PER_LANE];
#pragma unroll
    for (int r = 0; r < DTW_ROWS_PER_LANE; ++r) word[r] = 0u;
    // x of the cells of diagonal k (lane's rows i = 1 + lane + 64 r), fetched one diagonal ahead
    auto fetch = [&](int k) {
#pragma unroll
        for (int r = 0; r < DTW_ROWS_PER_LANE; ++r) {
            const int i = 1 + lane + 64 * r, j = k - i;
            xn[r] = (i <= N && j >= 1 && j <= M) ? xb[(long)(i - 1) * ld + (j - 1)] : 0.f;
        }
    };
    fetch(2);
    __syncthreads();
    for (int k = 2; k <= N + M; ++k) {
        float xc[DTW_ROWS_PER_LANE];
#pragma unroll
        for (int r = 0; r < DTW_ROWS_PER_LANE; ++r) xc[r] = xn[r];
        if (k < N + M) fetch(k + 1);
        float *Dk = D + (k % 3) * (N + 1);
        const float *D1 = D + ((k - 1) % 3) * (N + 1), *D2 = D + ((k - 2) % 3) * (N + 1);
#pragma unroll
        for (int r = 0; r < DTW_ROWS_PER_LANE; ++r) {
            const int i = 1 + lane + 64 * r, j = k - i;
            if (i <= N && j >= 1 && j <= M) {
                int t;
                Dk[i] = wm_dtw_cell(xc[r], D2[i - 1], D1[i - 1], D1[i], &t);
                word[r] |= (unsigned)t << (2 * ((j - 1) & 15));
                if (((j - 1) & 15) == 15 || j == M) {
                    tr[(long)(i - 1) * W + (j - 1) / 16] = word[r];
                    word[r] = 0u;
                }
            }
        }
        if (lane == 0) Dk[0] = INFINITY;          // cost[0][k]
        if (lane == 0 && k <= N) Dk[k] = INFINITY;   // cost[k][0]
        __syncthreads();
    }
    if (lane == 0) {
        int i = N, j = M;
        while (i > 0 || j > 0) {
            const int t = i == 0 ? 2 : j == 0 ? 1 : (int)((tr[(long)(i - 1) * W + (j - 1) / 16] >> (2 * ((j - 1) & 15))) & 3u);
            int row, frame;
            wm_dtw_move(t, &i, &j, &row, &frame);
            if (row >= 0) out[row] = frame;
        }
    }
}

}  // namespace

int wm_align_capture_q(wm_ctx *ctx, const float *dq, int d, int B, const WmAlignLayer &L, float *cap, int Tq, int J,
                       const int *pos_ptr, int panel, int base) {
    if (L.n <= 0) return WM_OK;
    WM_REQUIRE(panel >= 1 && panel <= WM_MAX_TEACHER_PANEL && B % panel == 0, WM_ERR_INVALID, "align_capture: %d rows in panels of %d", B, panel);
    WM_REQUIRE(base < 0 || panel == 1, WM_ERR_INVALID, "align_capture: a capture base goes with single steps");
    WmProfScope ps(&ctx->prof, "align_capture", ctx->stream);
    if (base >= 0) align_capture_kernel<false, true><<<dim3(B, L.n), 64, 0, ctx->stream>>>(dq, d, pos_ptr, L, cap, Tq, J, base);
    else if (panel > 1) align_capture_kernel<true><<<dim3(B, L.n), 64, 0, ctx->stream>>>(dq, d, pos_ptr, L, cap, Tq, J, panel);
    else align_capture_kernel<false><<<dim3(B, L.n), 64, 0, ctx->stream>>>(dq, d, pos_ptr, L, cap, Tq, J, 1);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_align_gather(wm_ctx *ctx, const float *cap, float *q_sel, const int *slot, const int *n_rows, int C, int N, int Tq, int J) {
    WM_REQUIRE(cap && q_sel && slot && n_rows && C >= 1 && N >= 1 && C * N <= WM_DEC_MAXB && Tq >= 1 && Tq <= AL_MAXT && J >= 1,
               WM_ERR_INVALID, "align_gather: bad geometry");
    WM_REQUIRE(((uintptr_t)cap | (uintptr_t)q_sel) % 16 == 0, WM_ERR_INVALID, "align_gather: buffers not 16-byte aligned");
    WmProfScope ps(&ctx->prof, "align_gather", ctx->stream);
    align_gather_kernel<<<dim3((Tq + AL_GATHER_ROWS - 1) / AL_GATHER_ROWS, C), 256, 0, ctx->stream>>>(
        (const uint4 *)cap, (uint4 *)q_sel, slot, n_rows, N, Tq, J);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_align_token_prob(wm_ctx *ctx, const float *logits, long ldo, const int *seq, const int *pos_ptr, int B, int S, int eot,
                        const int *n_text, float *prob, int max_text, int panel, int seq_stride) {
    WM_REQUIRE(panel >= 1 && panel <= WM_MAX_TEACHER_PANEL && B % panel == 0, WM_ERR_INVALID, "align_token_prob: %d rows in panels of %d", B, panel);
    WmProfScope ps(&ctx->prof, "align_token_prob", ctx->stream);
    const int stride = seq_stride > 0 ? seq_stride : B / panel;
    if (panel > 1) align_token_prob_kernel<true><<<B, 256, 0, ctx->stream>>>(logits, ldo, seq, pos_ptr, stride, S, eot, n_text, prob, max_text, panel);
    else align_token_prob_kernel<false><<<B, 256, 0, ctx->stream>>>(logits, ldo, seq, pos_ptr, stride, S, eot, n_text, prob, max_text, 1);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_align_matrix(wm_ctx *ctx, const WmAlignDev &a, int max_n, int max_m) {
    WM_REQUIRE(a.half >= 0 && a.half <= AL_MAXHALF, WM_ERR_INVALID, "align: median filter half-width %d > %d", a.half,
               AL_MAXHALF);
    WM_REQUIRE(a.Tq <= AL_MAXT, WM_ERR_INVALID, "align: %d decoder rows > %d", a.Tq, AL_MAXT);
    WM_REQUIRE((a.tail == 0 || a.tail == 1) && (a.n_min == 0 || a.n_min == 1), WM_ERR_INVALID, "align: row rule (%d, %d)", a.tail, a.n_min);
    if (max_n < a.n_min || max_m <= 0) return WM_OK;
    {
        WmProfScope ps(&ctx->prof, "align_stats", ctx->stream);
        align_stats_kernel<<<dim3(a.J, a.B), 256, 0, ctx->stream>>>(a);
        WM_HIP(hipGetLastError());
    }
    WmProfScope ps(&ctx->prof, "align_matrix", ctx->stream);
    const dim3 grid((max_m + AL_OUT - 1) / AL_OUT, (max_n + 1 + 15) / 16, a.B);
    if (a.half <= 3)
        align_matrix_kernel<7><<<grid, 256, 0, ctx->stream>>>(a);
    else
        align_matrix_kernel<0><<<grid, 256, 0, ctx->stream>>>(a);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

size_t wm_dtw_trace_words(int max_rows) { return (size_t)max_rows * ((1500 + 15) / 16); }

int wm_dtw(wm_ctx *ctx, const float *x, long x_bstride, int ld, const int *N, const int *M, int B, int max_rows, int max_m,
           unsigned *trace, int *start, int n_out) {
    WM_REQUIRE(max_rows >= 0 && max_rows <= DTW_ROWS_PER_LANE * 64 && max_m >= 0 && max_m <= 1500, WM_ERR_INVALID,
               "dtw: at most %d rows and 1500 frames", DTW_ROWS_PER_LANE * 64);
    WmProfScope ps(&ctx->prof, "align_dtw", ctx->stream);
    const size_t lds_cost = (size_t)3 * (max_rows + 1) * 4;
    const size_t lds_trace = (size_t)max_rows * ((max_m + 15) / 16) * 4;
    if (lds_cost + lds_trace <= 160 * 1024) {
        static bool attr = false;
        if (!attr) {
            WM_HIP(hipFuncSetAttribute((const void *)dtw_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr = true;
        }
        dtw_kernel<true><<<B, 64, lds_cost + lds_trace, ctx->stream>>>(x, x_bstride, ld, N, M, trace, 0, start, n_out);
    } else {
        dtw_kernel<false><<<B, 64, lds_cost, ctx->stream>>>(x, x_bstride, ld, N, M, trace, (long)wm_dtw_trace_words(max_rows),
                                                            start, n_out);
    }
    WM_HIP(hipGetLastError());
    return WM_OK;
}
