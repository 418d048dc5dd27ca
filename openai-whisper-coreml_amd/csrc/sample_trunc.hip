// sample_trunc.hip -- the sampling rules (wm_set_sampling_rules): top-k, top-p and min-p truncation of a
// sampling row's distribution, one launch per generated position between the DE_LOGITS_X* product (which stored the f32 row,
// penalised and biased, and left the per-tile partials) and the close.  One 16-wave workgroup per row:
//   * `forced` and the best value from the partials, and the admissible set: stored_row.h, shared with the other stored-row kernels;
//   * the cut: an LDS histogram (count and fixed-point mass per bin) over the top 11 bits of the order-preserving value word,
//     a walk from the top bin, the bin of the cut refined on the next 11 and the last 10 bits, ties at the cut by lowest id;
//   * the draw over the kept ids alone: philox.h's functions with the epilogue's counters, the epilogue's score and key;
//   * the hand-over (stored_row.h row_hand_over): the row's per-tile keys and winner values rewritten so that only the drawn id
//     is left.  The log-sum-exp partials stay, so argmax_embed_body and dec_close.h run unchanged and the log-prob is the
//     untruncated one.
// Everything order-dependent is integer: masses are u64 fixed point rint(m 2^40) (at most 131 072 terms <= 2^40), counts are
// integers, keys are compared, so the kept set and the token depend on the row's values, ids and seed alone.
#include "dec_close.h"
#include "model.h"
#include "philox.h"
#include "stored_row.h"

namespace {

constexpr int ST_THREADS = 1024, ST_BINS = 2048;
constexpr int ST_COUNT = 0, ST_MASS = 1;

// what a thread needs to walk row b: the stored values, the admissible set A and the mass of an id
struct StRow {
    const float *lg;
    RowAdmit adm;
    float vmax, inv_T;
    // m(n) = exp((v - vmax) inv_T), and its fixed-point form
    __device__ __forceinline__ float mass(float v) const { return v == vmax ? 1.f : __expf((v - vmax) * inv_T); }
    __device__ __forceinline__ unsigned long long mass_fix(float v) const { return __float2ull_rn(mass(v) * 1099511627776.f); }
};
// f(n, v, u) for every id of A whose value is above -inf (-inf and NaN are never kept); u = the value word of argmax_key
template <class F>
__device__ __forceinline__ void st_for_each(const StRow &r, F f) {
    row_for_each_admitted(r.lg, r.adm, [&](int n, float v) {
        if (v > -INFINITY) f(n, v, (unsigned)(argmax_key(v, n) >> 32));
    });
}

struct StFound {
    int bin;   // -1: no bin holds the target
    unsigned c_before, c_bin, c_total;
    unsigned long long m_before, m_bin, m_total;
};
struct StShared {
    unsigned cnt[ST_BINS];
    unsigned long long mass[ST_BINS];
    unsigned cnt0[ST_BINS];              // the level-0 histogram, kept for a second descent
    unsigned long long mass0[ST_BINS];
    unsigned wc[16];
    unsigned long long wm[16], red[16];
    StFound found;
    int tie_id, kept;
};

__device__ __forceinline__ void st_hist_clear(StShared &s) {
    for (int i = threadIdx.x; i < ST_BINS; i += ST_THREADS) { s.cnt[i] = 0u; s.mass[i] = 0ull; }
    __syncthreads();
}
__device__ __forceinline__ void st_hist_copy(StShared &s, bool save) {
    for (int i = threadIdx.x; i < ST_BINS; i += ST_THREADS) {
        if (save) { s.cnt0[i] = s.cnt[i]; s.mass0[i] = s.mass[i]; }
        else { s.cnt[i] = s.cnt0[i]; s.mass[i] = s.mass0[i]; }
    }
    __syncthreads();
}
// Level `level` of the value word, over the ids whose higher bits equal `prefix`: 11 | 11 | 10 bits.
__device__ __forceinline__ void st_hist_values(StShared &s, const StRow &r, int level, unsigned prefix) {
    st_hist_clear(s);
    st_for_each(r, [&](int, float v, unsigned u) {
        unsigned bin;
        if (level == 0) bin = u >> 21;
        else if (level == 1) { if ((u >> 21) != prefix) return; bin = (u >> 10) & 2047u; }
        else { if ((u >> 10) != prefix) return; bin = u & 1023u; }
        atomicAdd(&s.cnt[bin], 1u);
        const unsigned long long mf = r.mass_fix(v);
        if (mf) atomicAdd(&s.mass[bin], mf);
    });
    __syncthreads();
}
// The walk: bins in descending (desc) or ascending order; the bin in which the running count (ST_COUNT) or mass (ST_MASS)
// first reaches `target` >= 1, with what lies in front of it, and the totals.  Integer adds: any order, same result.
__device__ __forceinline__ StFound st_hist_find(StShared &s, bool desc, int mode, unsigned long long target) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = desc ? ST_BINS - 1 - 2 * tid : 2 * tid, b1 = desc ? b0 - 1 : b0 + 1;
    const unsigned c0 = s.cnt[b0], c1 = s.cnt[b1];
    const unsigned long long m0 = s.mass[b0], m1 = s.mass[b1];
    unsigned ic = c0 + c1;
    unsigned long long im = m0 + m1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned tc = __shfl_up(ic, o);
        const unsigned long long tm = __shfl_up(im, o);
        if (lane >= o) { ic += tc; im += tm; }
    }
    if (lane == 63) { s.wc[wave] = ic; s.wm[wave] = im; }
    if (tid == 0) s.found.bin = -1;
    __syncthreads();
    unsigned pc = 0u, tc = 0u;
    unsigned long long pm = 0ull, tm = 0ull;
    for (int w = 0; w < 16; ++w) {
        const unsigned c = s.wc[w];
        const unsigned long long m = s.wm[w];
        if (w < wave) { pc += c; pm += m; }
        tc += c; tm += m;
    }
    const unsigned ec = pc + ic - (c0 + c1);
    const unsigned long long em = pm + im - (m0 + m1);
    auto test = [&](int bin, unsigned cb, unsigned long long mb, unsigned c, unsigned long long m) {
        const bool hit = mode == ST_COUNT ? (c > 0u && (unsigned long long)cb < target && target <= (unsigned long long)cb + c)
                                          : (m > 0ull && mb < target && target <= mb + m);
        if (hit) { s.found.bin = bin; s.found.c_before = cb; s.found.c_bin = c; s.found.m_before = mb; s.found.m_bin = m; }
    };
    test(b0, ec, em, c0, m0);
    test(b1, ec + c0, em + m0, c1, m1);
    if (tid == 0) { s.found.c_total = tc; s.found.m_total = tm; }
    __syncthreads();
    const StFound f = s.found;
    __syncthreads();
    return f;
}

// the r-th (1-based) lowest id among the ids of A whose value word is u: a histogram over id >> sh, an ascending walk, and
// one ballot over the <= 64 ids of the bin
__device__ __forceinline__ int st_tie_select(StShared &s, const StRow &r, unsigned u_cut, unsigned rth) {
    int sh = 0;
    while (((r.adm.V - 1) >> sh) >= ST_BINS) ++sh;   // (the launch checks V <= 64 ST_BINS)
    st_hist_clear(s);
    st_for_each(r, [&](int n, float, unsigned u) { if (u == u_cut) atomicAdd(&s.cnt[n >> sh], 1u); });
    __syncthreads();
    const StFound f = st_hist_find(s, false, ST_COUNT, rth);
    if (threadIdx.x == 0) s.tie_id = -1;
    __syncthreads();
    if (f.bin >= 0 && threadIdx.x < 64) {
        const int n = (f.bin << sh) + (int)threadIdx.x;
        bool is = false;
        if ((int)threadIdx.x < (1 << sh) && n < r.adm.V && row_admits(r.adm, n)) {
            const float v = r.lg[n];
            is = v > -INFINITY && (unsigned)(argmax_key(v, n) >> 32) == u_cut;
        }
        const unsigned long long bal = __ballot(is);
        if (is && (unsigned)__popcll(bal & ((1ull << threadIdx.x) - 1ull)) == rth - f.c_before - 1u) s.tie_id = n;
    }
    __syncthreads();
    const int id = s.tie_id;
    __syncthreads();
    return id;
}

// The shortest prefix of A, in descending key order, whose count (ST_COUNT) or mass (ST_MASS) reaches `target`: the prefix is
// the ids with argmax_key >= key; mass = its fixed-point mass.  have0: the level-0 histogram is in place.
struct StCut {
    unsigned long long key, mass;
};
__device__ __forceinline__ StCut st_descend(StShared &s, const StRow &r, int mode, unsigned long long target, bool have0) {
    unsigned long long bc = 0ull, bm = 0ull;
    unsigned prefix = 0u;
    StFound f;
    for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0), bits = level == 2 ? 10 : 11;
        if (!(level == 0 && have0)) st_hist_values(s, r, level, prefix);
        const unsigned long long rem = target - (mode == ST_COUNT ? bc : bm);
        f = st_hist_find(s, true, mode, rem);
        if (f.bin < 0) return StCut{1ull, bm + f.m_total};   // (a target above the total: everything)
        bc += f.c_before; bm += f.m_before;
        prefix = (prefix << bits) | (unsigned)f.bin;
        // the cut falls on the bin's lower edge: no finer look is needed
        const bool whole = mode == ST_COUNT ? (rem - f.c_before == f.c_bin) : (f.c_bin == 1u);
        if (whole) return StCut{(unsigned long long)(prefix << shift) << 32, bm + f.m_bin};
    }
    // ties: f.c_bin ids with the value word `prefix`, every one of the same mass; the lowest ids are kept
    const unsigned long long mt = f.m_bin / f.c_bin;
    unsigned long long need = mode == ST_COUNT ? target - bc : (mt ? (target - bm + mt - 1ull) / mt : (unsigned long long)f.c_bin);
    if (need >= f.c_bin) return StCut{(unsigned long long)prefix << 32, bm + f.m_bin};
    if (need < 1ull) need = 1ull;
    const int id = st_tie_select(s, r, prefix, (unsigned)need);
    if (id < 0) return StCut{(unsigned long long)prefix << 32, bm + f.m_bin};
    return StCut{((unsigned long long)prefix << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)id), bm + need * mt};
}

__device__ __forceinline__ unsigned long long st_block_max(StShared &s, unsigned long long k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    k = key_max_xor<64>(k);
    if (lane == 0) s.red[wave] = k;
    __syncthreads();
    unsigned long long r = lane < 16 ? s.red[lane] : 0ull;
    r = __shfl(key_max_xor<16>(r), 0);
    __syncthreads();
    return r;
}

// dbg (nullable): [rows][3] kept ids, the last kept id, the drawn id (0, -1, -1: the row was left alone)
__global__ __launch_bounds__(ST_THREADS) void sample_trunc_kernel(const float *__restrict__ logits, long ldo, int V, int n_tiles,
                                                                  unsigned long long *__restrict__ tilemax, WmTsDev ts, WmXDev xd,
                                                                  const unsigned *__restrict__ mask, int mask_words, int n_prompt,
                                                                  const int *__restrict__ pos_ptr, const int *__restrict__ done,
                                                                  const unsigned *__restrict__ ban, int ban_words,
                                                                  const WmSampPar *__restrict__ par, int *__restrict__ dbg) {
    __shared__ StShared s;
    __shared__ float seg_s[16][4];
    __shared__ int forced_s;
    __shared__ float vmax_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int pos = *pos_ptr;
    const WmXPar xp = *xd.par;
    const WmSampPar sp = *par;
    const int gi = pos + 1 - xp.n_prompt;
    if (dbg && threadIdx.x == 0) { dbg[b * 3] = 0; dbg[b * 3 + 1] = -1; dbg[b * 3 + 2] = -1; }
    // workgroup-uniform: a prompt position, an arg-max call, a row that is done (a window that has left: its rows are done)
    if (gi < 0 || !xp.sample || (done && done[b])) return;
    // the row's own 1 / T and key under a row table (wm_set_sampling_rows); an arg-max row of it is left alone (uniform)
    float inv_T = xp.inv_T;
    unsigned key0 = xp.key0, key1 = xp.key1;
    if (xp.rows_on) {
        const WmXRow rw = wm_x_rows(xd.ids)[b];
        inv_T = rw.inv_T; key0 = rw.key0; key1 = rw.key1;
        if (__float_as_uint(inv_T) == 0u) return;
    }
    const long rb = (long)b * n_tiles;
    // `forced` (the sum rule) and the best value of A, from the partials
    stored_row_prologue(ts, xd, tilemax, b, n_tiles, false, seg_s, s.red, [&](const RowChoice &ch, Lse lt, Lse) {
        if (lane == 0) {
            forced_s = ch.forced ? 1 : 0;
            vmax_s = row_best_value(ch, lt);
        }
    });
    const bool forced = forced_s != 0;
    if (!(vmax_s > -1e30f)) return;   // nothing to keep: the close takes its existing path (uniform)
    StRow r;
    r.lg = logits + (long)b * ldo;
    r.adm = row_admit_set(V, ts, mask, mask_words, ban, ban_words, b, pos, n_prompt, forced);
    r.vmax = vmax_s;
    r.inv_T = inv_T;
    // the cut
    unsigned long long cut = 1ull;   // every key of A is at or above it
    const bool p_on = sp.top_p < 1.f;
    if (sp.top_k > 0 || p_on) {
        st_hist_values(s, r, 0, 0u);
        const StFound all = st_hist_find(s, true, ST_COUNT, 1ull);   // (for the totals)
        unsigned long long zk = all.m_total;
        const bool have0 = true;
        if (sp.top_k > 0 && (unsigned)sp.top_k < all.c_total) {
            if (p_on) st_hist_copy(s, true);    // (the second descent starts from the same level 0)
            const StCut c = st_descend(s, r, ST_COUNT, (unsigned long long)sp.top_k, have0);
            cut = c.key > cut ? c.key : cut;
            zk = c.mass;
            if (p_on) st_hist_copy(s, false);
        }
        if (p_on && zk > 0ull) {
            const double want = ceil((double)sp.top_p * (double)zk);
            unsigned long long target = want < 1.0 ? 1ull : (unsigned long long)want;
            target = target > zk ? zk : target;
            const StCut c = st_descend(s, r, ST_MASS, target, have0);
            cut = c.key > cut ? c.key : cut;
        }
    }
    // the draw over the kept ids: the epilogue's counters, score and key; one Philox call serves the four ids of a quad
    unsigned long long best = 0ull, low = ~0ull;
    float best_v = 0.f;
    int kept = 0;
    const unsigned cw2 = xp.ids_on ? xd.ids[b] : (unsigned)(xp.chunk0 + b);
    const unsigned cw3 = xp.n_cand > 1 ? xd.ids[WM_XIDS_CAND + b] : 0u;
    constexpr int QU = 2;   // quads in flight per thread: their loads are requested together (see row_for_each_admitted)
    for (int q0 = threadIdx.x; q0 * 4 < V; q0 += ST_THREADS * QU) {
        float vq[QU][4];
        unsigned wq[QU];
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int q = q0 + u * ST_THREADS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = q * 4 + j;
                vq[u][j] = r.lg[n < V ? n : V - 1];   // (clamped: dropped below)
            }
            const int wn = q * 4 < V ? q * 4 : V - 1;   // (the four ids of a quad share a bitmap word)
            wq[u] = (r.adm.mrow ? r.adm.mrow[wn >> 5] : 0u) | (r.adm.brow ? r.adm.brow[wn >> 5] : 0u);
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int q = q0 + u * ST_THREADS;
            bool have = false;
            wm_philox4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = q * 4 + j;
                const float v = vq[u][j];
                if (n >= V || !row_in_ranges(r.adm, n) || ((wq[u] >> (n & 31)) & 1u) || !(v > -INFINITY)) continue;
                const unsigned long long k = argmax_key(v, n);
                if (k < cut || (sp.min_p > 0.f && !(r.mass(v) >= sp.min_p))) continue;
                if (!have) {
                    wm_philox4 c;
                    c.v[0] = (unsigned)q; c.v[1] = (unsigned)gi; c.v[2] = cw2; c.v[3] = cw3;
                    w = wm_philox4x32_10(c, key0, key1);
                    have = true;
                }
                const float sc = __fmaf_rn(v, inv_T, wm_gumbel_from_bits(wm_philox_word(w, (unsigned)j)));
                const unsigned long long sk = argmax_key(sc, n);
                if (sk > best) { best = sk; best_v = v; }
                low = k < low ? k : low;
                ++kept;
            }
        }
    }
    if (threadIdx.x == 0) s.kept = 0;
    __syncthreads();
    if (kept) atomicAdd(&s.kept, kept);
    const unsigned long long win = st_block_max(s, best);
    const unsigned long long last = ~st_block_max(s, ~low);
    if (win == 0ull) return;   // (cannot happen: the best id of A is always kept)
    // the hand-over: only the drawn id is left in the row's keys
    const int tok = argmax_key_index(win);
    row_hand_over(ts, tilemax, rb, n_tiles, forced, win, threadIdx.x, ST_THREADS);
    if (best == win) xd.win[row_win_slot(ts, rb, tok)] = best_v;   // (keys carry the id: one thread)
    if (dbg && threadIdx.x == 0) { dbg[b * 3] = s.kept; dbg[b * 3 + 1] = argmax_key_index(last); dbg[b * 3 + 2] = tok; }
}

}  // namespace

int wm_sample_truncate(wm_ctx *ctx, const WmStoredRows &r, const WmSampPar *par, int *dbg) {
    WmProfScope ps(&ctx->prof, "sample_trunc", ctx->stream);
    WM_TRY(wm_stored_rows_check(r, "sample_truncate", true));
    WM_REQUIRE(par, WM_ERR_INVALID, "sample_truncate: no rules");
    WM_REQUIRE(r.n_vocab <= 64 * ST_BINS, WM_ERR_INVALID, "sample_truncate: %d ids outside 1 .. %d", r.n_vocab, 64 * ST_BINS);
    sample_trunc_kernel<<<r.rows, ST_THREADS, 0, ctx->stream>>>(r.logits, r.ldo, r.n_vocab, (r.n_vocab + 15) / 16, r.tilemax, r.ts, r.xd,
                                                               r.mask, r.mask_words, r.n_prompt, r.pos_ptr, r.stop.done, r.ban, r.ban_words,
                                                               par, dbg);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
