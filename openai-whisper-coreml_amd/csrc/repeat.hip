// repeat.hip -- the repetition rules (wm_set_repetition_rules): the per-row state the DE_LOGITS_XR
// epilogue and the beam list kernel read.
//
// wm_repeat_state runs once per decode position, in line on the group's stream in front of the logits GEMV, and REBUILDS
// two bitmaps over the vocabulary for every row from the row's generated history g[0 .. k) (positions n_prompt .. pos of
// the token buffer [T][B]; the prompt is excluded):
//   seen: ids < eot that occur in g                                   (the repetition penalty applies to them, once each)
//   ban : ids t < eot for which some i in [0, k - n] has g[i .. i + n - 1) == g[k - n + 1 .. k) and g[i + n - 1] == t
//                                                                      (no_repeat_ngram_size = n; n = 1: ban == seen)
// Rebuilding instead of updating is deliberate: after a beam re-parenting a row's history is another row's, and a finished
// row, a ragged row or a replayed graph needs no case of its own -- a stale bit cannot exist.  The work is tiny (<= 448
// tokens, <= 31 comparisons per start) next to the 13 KB of bitmap a row writes; both bitmaps are built in LDS with
// atomicOr and leave as plain coalesced dword stores.
#include "model.h"

namespace {
constexpr int kThreads = 256;

// grid: B rows.  Dynamic LDS: seen [words] | ban [words] | g [n_ctx] (32-bit words)
__global__ __launch_bounds__(kThreads) void repeat_state_kernel(const int *__restrict__ seq, const int *__restrict__ pos_ptr, int B,
                                                                int n_prompt, int n_ctx, int V, WmRepDev rep) {
    extern __shared__ unsigned rs_smem[];
    unsigned *seen = rs_smem, *ban = rs_smem + rep.words;
    int *g = (int *)(rs_smem + 2 * rep.words);
    const int b = blockIdx.x, tid = threadIdx.x;
    const WmRepPar par = *rep.par;
    int k = *pos_ptr + 1 - n_prompt;   // generated tokens so far (a prompt position: none)
    k = k < 0 ? 0 : k;
    k = k > n_ctx - n_prompt ? n_ctx - n_prompt : k;
    const int lim = par.eot < V ? par.eot : V;   // eligible ids: [0, lim)
    for (int w = tid; w < 2 * rep.words; w += kThreads) rs_smem[w] = 0u;
    for (int i = tid; i < k; i += kThreads) g[i] = seq[(long)(n_prompt + i) * B + b];
    __syncthreads();
    for (int i = tid; i < k; i += kThreads) {
        const int t = g[i];
        if (t >= 0 && t < lim) atomicOr(&seen[t >> 5], 1u << (t & 31));
    }
    const int n = par.n;
    if (n >= 1) {
        const int s0 = k - n + 1;   // the suffix = the last n - 1 tokens, g[s0 .. k) (read only when a start exists: k >= n)
        for (int i = tid; i <= k - n; i += kThreads) {
            const int t = g[i + n - 1];
            if (t < 0 || t >= lim) continue;
            bool same = true;
            for (int j = 0; j < n - 1; ++j) same = same && g[i + j] == g[s0 + j];
            if (same) atomicOr(&ban[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
    unsigned *so = rep.seen + (long)b * rep.words, *bo = rep.ban + (long)b * rep.words;
    for (int w = tid; w < rep.words; w += kThreads) {
        so[w] = seen[w];
        bo[w] = ban[w];
    }
}
}  // namespace

int wm_repeat_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmRepDev &rep) {
    WM_REQUIRE(seq && pos_ptr && rep.par && rep.seen && rep.ban, WM_ERR_INVALID, "repeat_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && n_prompt >= 0 && n_ctx >= 1 && n_prompt <= n_ctx && V >= 1 && rep.words >= 1 &&
                   (long)rep.words * 32 >= V,
               WM_ERR_INVALID, "repeat_state: bad shape (B %d, prompt %d of %d, V %d, %d words)", B, n_prompt, n_ctx, V, rep.words);
    const size_t lds = ((size_t)2 * rep.words + n_ctx) * 4;
    WM_REQUIRE(lds <= 64 * 1024, WM_ERR_INVALID, "repeat_state: a vocabulary of %d ids does not fit the bitmaps' 64 KiB of LDS", V);
    WmProfScope ps(&ctx->prof, "repeat_state", ctx->stream);
    repeat_state_kernel<<<B, kThreads, lds, ctx->stream>>>(seq, pos_ptr, B, n_prompt, n_ctx, V, rep);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
