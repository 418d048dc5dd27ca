// seqbias.hip -- the sequence bias (wm_set_sequence_bias): the per-row state the DE_LOGITS_XB epilogue
// reads.
//
// wm_seqbias_state runs once per decode position, in line on the group's stream behind wm_repeat_state and in front of the
// logits GEMV, and REBUILDS for every row, from the row's generated history g[0 .. k) (positions n_prompt .. pos of the token
// buffer [T][B]; the prompt is excluded):
//   hit : the ids t for which at least one table entry with last token t matches -- n == 1, or k >= n - 1 and
//         g[k - n + 1 .. k) == s[0 .. n - 1)
//   list: (id, total) of exactly those ids, ascending by id, total = the f32 sum from +0.0f of the matching entries' biases in
//         table order; cnt = its length
//   woff: per bitmap word the number of hit bits in the words below it = the list index of the word's first hit id, so the
//         epilogue finds an id's total at woff[word] + popcount(hit bits below it): ONE load, no search
//   ban : the ids whose total is -inf, OR-ed into the words wm_repeat_state has just rebuilt (they are in hit and the list too:
//         the stored logit is v + total = -inf, the ban bit keeps the id out of the allowed set)
// The table arrives sorted by last token (wm_sb_expand): the entries of one id are a contiguous GROUP in given order, the
// groups ascend by id.  One lane takes one group and sums it sequentially -- the order of the sum is the table's, whatever the
// launch looks like --; an entry's context is stored newest token first and compared against the history from the newest
// token backwards, so nearly every entry fails at its first comparison.  A matched group's place in the list is the rank of
// its id among the hit bits (the groups' ids are distinct): no atomics on the order, no sort.
// Rebuilding instead of updating: as wm_repeat_state (a re-parented, finished or ragged row needs no case of its own).
#include "model.h"

namespace {
constexpr int kThreads = 1024;   // 4096 groups: four per lane, each a chain of dependent loads (with 256 lanes the launch took 23 - 29 us, now 12 - 14)
constexpr int kWaves = kThreads / 64;
constexpr int kCap = WM_MAX_BIAS_ENTRIES;
constexpr int kFlagWords = kCap / 32;

// grid: B rows.  Dynamic LDS (32-bit words): hit [words] | ban [words] | woff [words] | tot [kCap] | flag [128] | h [32] | wsum [kWaves + 1]
__global__ __launch_bounds__(kThreads) void seqbias_state_kernel(const int *__restrict__ seq, const int *__restrict__ pos_ptr, int B,
                                                                 int n_prompt, int n_ctx, int V, WmSbDev sb, unsigned *__restrict__ ban,
                                                                 int ban_words) {
    extern __shared__ unsigned sb_smem[];
    const int words = sb.e.words;   // <= 2 * kThreads (the launcher checks): two words per lane in the prefix sums
    unsigned *hitl = sb_smem, *banl = sb_smem + words, *woffl = sb_smem + 2 * words;
    float *tot = (float *)(sb_smem + 3 * words);
    unsigned *flag = sb_smem + 3 * words + kCap;
    int *h = (int *)(flag + kFlagWords);
    unsigned *wsum = (unsigned *)(h + 32);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const WmSbPar par = *sb.par;
    int k = *pos_ptr + 1 - n_prompt;   // generated tokens so far (a prompt position: none)
    k = k < 0 ? 0 : k;
    k = k > n_ctx - n_prompt ? n_ctx - n_prompt : k;
    const int nh = k < WM_SB_CTX ? k : WM_SB_CTX;   // the newest tokens an entry can ask for
    const int ng = par.n_groups < kCap ? (par.n_groups < 0 ? 0 : par.n_groups) : kCap;
    const int lim = V < words * 32 ? V : words * 32;
    for (int w = tid; w < 2 * words; w += kThreads) sb_smem[w] = 0u;
    if (tid < kFlagWords) flag[tid] = 0u;
    if (tid < nh) h[tid] = seq[(long)(n_prompt + k - 1 - tid) * B + b];   // h[j] = g[k - 1 - j]
    __syncthreads();
    for (int g = tid; g < ng; g += kThreads) {
        const int id = sb.grp_id[g];
        int e0 = sb.grp_beg[g], e1 = sb.grp_beg[g + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > kCap ? kCap : e1;
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
            tot[g] = total;
            atomicOr(&flag[g >> 5], 1u << (g & 31));
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
    for (int g = tid; g < ng; g += kThreads) {
        if (!((flag[g >> 5] >> (g & 31)) & 1u)) continue;
        const int id = sb.grp_id[g];   // (in [0, lim): flagged above)
        const unsigned at = woffl[id >> 5] + __popc(hitl[id >> 5] & ((1u << (id & 31)) - 1u));   // < kCap: at most ng distinct ids are hit
        if (at < (unsigned)kCap) {
            lid[at] = id;
            ltot[at] = tot[g];
        }
    }
    if (tid == 0) sb.e.cnt[b] = (int)wsum[kWaves];
    unsigned *ho = sb.e.hit + (long)b * words, *bo = ban + (long)b * ban_words;
    int *wo = sb.e.woff + (long)b * words;
    for (int w = tid; w < words; w += kThreads) {
        ho[w] = hitl[w];
        wo[w] = (int)woffl[w];
        const unsigned bw = banl[w];
        if (bw && w < ban_words) bo[w] = bo[w] | bw;   // one workgroup owns the row: a plain read-modify-write
    }
}
}  // namespace

int wm_seqbias_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmSbDev &sb,
                     unsigned *ban, int ban_words) {
    WM_REQUIRE(seq && pos_ptr && ban && sb.par && sb.grp_id && sb.grp_beg && sb.ent_len && sb.ent_bias && sb.ent_ctx && sb.e.hit &&
                   sb.e.cnt && sb.e.lid && sb.e.ltot && sb.e.woff,
               WM_ERR_INVALID, "seqbias_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && n_prompt >= 0 && n_ctx >= 1 && n_prompt <= n_ctx && V >= 1 && sb.e.words >= 1 &&
                   (long)sb.e.words * 32 >= V && ban_words >= sb.e.words && sb.e.words <= 2 * kThreads,
               WM_ERR_INVALID, "seqbias_state: bad shape (B %d, prompt %d of %d, V %d, %d / %d words)", B, n_prompt, n_ctx, V, sb.e.words,
               ban_words);
    const size_t lds = ((size_t)3 * sb.e.words + kCap + kFlagWords + 32 + kWaves + 1) * 4;
    WM_REQUIRE(lds <= 64 * 1024, WM_ERR_INVALID, "seqbias_state: a vocabulary of %d ids does not fit the bitmaps' 64 KiB of LDS", V);
    WmProfScope ps(&ctx->prof, "seqbias_state", ctx->stream);
    seqbias_state_kernel<<<B, kThreads, lds, ctx->stream>>>(seq, pos_ptr, B, n_prompt, n_ctx, V, sb, ban, ban_words);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
