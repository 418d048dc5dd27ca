// seqbias_rows.hip -- the sequence bias with a table per row (wm_set_sequence_bias_tables / wm_set_bias_rows, DESIGN.md
// section 15): the per-row state the DE_LOGITS_XB epilogue reads, rebuilt from each row's OWN table.
//
// wm_seqbias_rows_state is wm_seqbias_state (seqbias.hip: read its header first) with one difference: the tables of the context
// are concatenated into a pool in the layout of WmSbDev -- grp_beg absolute into the pool's entries -- and row b walks only the
// groups [rng[2 b], rng[2 b + 1]) of it, its table's.  Everything else is that kernel's: one workgroup of 1024 lanes per row,
// rebuilt on every position from the generated history, in line behind wm_repeat_state (under beam search: behind the reorder),
// one lane per group summing it sequentially in table order -- so a row's totals are the single-table kernel's for that table,
// bit for bit --, the rank of a group's id among the hit bits as its place in the list, the bans OR-ed into wm_repeat_state's
// words.  Group g of the row is LOCAL group g - g0 in the LDS arrays (a table has at most WM_MAX_BIAS_ENTRIES groups).
// A row without a table (-1) or with an empty one has the empty range: an all-zero hit row, cnt = 0, and its ban words are not
// touched.
#include "model.h"

namespace {
constexpr int kThreads = 1024;   // as seqbias_state_kernel: 4096 groups, four per lane, each a chain of dependent loads
constexpr int kWaves = kThreads / 64;
constexpr int kCap = WM_MAX_BIAS_ENTRIES;   // groups (and entries) of ONE table
constexpr int kPool = WM_MAX_BIAS_POOL;     // groups (and entries) of the pool
constexpr int kFlagWords = kCap / 32;

// grid: B rows.  Dynamic LDS (32-bit words): hit [words] | ban [words] | woff [words] | tot [kCap] | flag [128] | h [32] | wsum [kWaves + 1]
__global__ __launch_bounds__(kThreads) void seqbias_rows_state_kernel(const int *__restrict__ seq, const int *__restrict__ pos_ptr, int B,
                                                                      int n_prompt, int n_ctx, int V, WmSbDev sb,
                                                                      const int *__restrict__ rng, unsigned *__restrict__ ban,
                                                                      int ban_words) {
    extern __shared__ unsigned sbr_smem[];
    const int words = sb.e.words;   // <= 2 * kThreads (the launcher checks): two words per lane in the prefix sums
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the row's groups of the pool, clamped to the pool and to one table's capacity
    int g0 = rng[2 * b], g1 = rng[2 * b + 1];
    g0 = g0 < 0 ? 0 : (g0 > kPool ? kPool : g0);
    g1 = g1 < g0 ? g0 : (g1 > kPool ? kPool : g1);
    const int ng = g1 - g0 < kCap ? g1 - g0 : kCap;
    unsigned *ho = sb.e.hit + (long)b * words;
    int *wo = sb.e.woff + (long)b * words;
    if (ng == 0) {   // (the whole workgroup: no table, or an empty one) nothing matches, the ban words stay wm_repeat_state's
        for (int w = tid; w < words; w += kThreads) {
            ho[w] = 0u;
            wo[w] = 0;
        }
        if (tid == 0) sb.e.cnt[b] = 0;
        return;
    }
    unsigned *hitl = sbr_smem, *banl = sbr_smem + words, *woffl = sbr_smem + 2 * words;
    float *tot = (float *)(sbr_smem + 3 * words);
    unsigned *flag = sbr_smem + 3 * words + kCap;
    int *h = (int *)(flag + kFlagWords);
    unsigned *wsum = (unsigned *)(h + 32);
    int k = *pos_ptr + 1 - n_prompt;   // generated tokens so far (a prompt position: none)
    k = k < 0 ? 0 : k;
    k = k > n_ctx - n_prompt ? n_ctx - n_prompt : k;
    const int nh = k < WM_SB_CTX ? k : WM_SB_CTX;   // the newest tokens an entry can ask for
    const int lim = V < words * 32 ? V : words * 32;
    for (int w = tid; w < 2 * words; w += kThreads) sbr_smem[w] = 0u;
    if (tid < kFlagWords) flag[tid] = 0u;
    if (tid < nh) h[tid] = seq[(long)(n_prompt + k - 1 - tid) * B + b];   // h[j] = g[k - 1 - j]
    __syncthreads();
    for (int gl = tid; gl < ng; gl += kThreads) {
        const int g = g0 + gl;   // < kPool
        const int id = sb.grp_id[g];
        int e0 = sb.grp_beg[g], e1 = sb.grp_beg[g + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > kPool ? kPool : e1;
        float total = 0.f;
        bool any = false;
        for (int e = e0; e < e1; ++e) {   // sequential, in table order: the order of the sum
            const int c = sb.ent_len[e];
            bool m = c >= 0 && c <= nh;
            const int *cx = sb.ent_ctx + (long)e * WM_SB_CTX;
            for (int j = 0; m && j < c; ++j) m = cx[j] == h[j];
            if (m) {
                total = __fadd_rn(total, sb.ent_bias[e]);
                any = true;
            }
        }
        if (any && id >= 0 && id < lim) {
            tot[gl] = total;
            atomicOr(&flag[gl >> 5], 1u << (gl & 31));
            atomicOr(&hitl[id >> 5], 1u << (id & 31));
            if (total == -INFINITY) atomicOr(&banl[id >> 5], 1u << (id & 31));
        }
    }
    __syncthreads();
    // exclusive prefix sums of the hit bits per word, two adjacent words per lane: wave scan, then the waves' sums
    const int w0 = 2 * tid, w1 = 2 * tid + 1;
    const unsigned a = w0 < words ? __popc(hitl[w0]) : 0u, c2 = w1 < words ? __popc(hitl[w1]) : 0u;
    unsigned incl = a + c2;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0u;
        for (int w = 0; w < kWaves; ++w) {
            const unsigned t = wsum[w];
            wsum[w] = run;
            run += t;
        }
        wsum[kWaves] = run;   // the list's length
    }
    __syncthreads();
    const unsigned excl = wsum[wave] + incl - (a + c2);
    if (w0 < words) woffl[w0] = excl;
    if (w1 < words) woffl[w1] = excl + a;
    __syncthreads();
    int *lid = sb.e.lid + (long)b * kCap;
    float *ltot = sb.e.ltot + (long)b * kCap;
    for (int gl = tid; gl < ng; gl += kThreads) {
        if (!((flag[gl >> 5] >> (gl & 31)) & 1u)) continue;
        const int id = sb.grp_id[g0 + gl];   // (in [0, lim): flagged above)
        const unsigned at = woffl[id >> 5] + __popc(hitl[id >> 5] & ((1u << (id & 31)) - 1u));   // < kCap: at most ng distinct ids are hit
        if (at < (unsigned)kCap) {
            lid[at] = id;
            ltot[at] = tot[gl];
        }
    }
    if (tid == 0) sb.e.cnt[b] = (int)wsum[kWaves];
    unsigned *bo = ban + (long)b * ban_words;
    for (int w = tid; w < words; w += kThreads) {
        ho[w] = hitl[w];
        wo[w] = (int)woffl[w];
        const unsigned bw = banl[w];
        if (bw && w < ban_words) bo[w] = bo[w] | bw;   // one workgroup owns the row: a plain read-modify-write
    }
}
}  // namespace

int wm_seqbias_rows_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmSbDev &pool,
                          const int *rng, unsigned *ban, int ban_words) {
    WM_REQUIRE(seq && pos_ptr && ban && rng && pool.grp_id && pool.grp_beg && pool.ent_len && pool.ent_bias && pool.ent_ctx &&
                   pool.e.hit && pool.e.cnt && pool.e.lid && pool.e.ltot && pool.e.woff,
               WM_ERR_INVALID, "seqbias_rows_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && n_prompt >= 0 && n_ctx >= 1 && n_prompt <= n_ctx && V >= 1 && pool.e.words >= 1 &&
                   (long)pool.e.words * 32 >= V && ban_words >= pool.e.words && pool.e.words <= 2 * kThreads,
               WM_ERR_INVALID, "seqbias_rows_state: bad shape (B %d, prompt %d of %d, V %d, %d / %d words)", B, n_prompt, n_ctx, V,
               pool.e.words, ban_words);
    const size_t lds = ((size_t)3 * pool.e.words + kCap + kFlagWords + 32 + kWaves + 1) * 4;
    WM_REQUIRE(lds <= 64 * 1024, WM_ERR_INVALID, "seqbias_rows_state: a vocabulary of %d ids does not fit the bitmaps' 64 KiB of LDS", V);
    WmProfScope ps(&ctx->prof, "seqbias_rows_state", ctx->stream);
    seqbias_rows_state_kernel<<<B, kThreads, lds, ctx->stream>>>(seq, pos_ptr, B, n_prompt, n_ctx, V, pool, rng, ban, ban_words);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
