// constraint.hip -- the constraint (wm_set_constraint): a token automaton masks each row on the device.
//
// wm_constraint_state runs once per decode position, in line on the group's stream behind wm_repeat_state (and the
// sequence-bias launch) and in front of the logits GEMV.  For every row whose start state is >= 0, at a position with k >= 0
// generated tokens, it REBUILDS from the row's generated history g[0 .. k) (positions n_prompt .. pos of the token buffer
// [T][B]; the prompt is excluded):
//   state  : s_k = fold delta over g from the row's start state.  delta(s, t) = s for t >= eot (timestamps, specials, the eot
//            padding of a finished row) and for s = -1; else the target of the explicit edge (s, t) if there is one, else
//            def_next[s]; a target of -1 -- a forbidden id -- is the dead state, which stays dead.
//   allowed: the ids of [0, eot] state s_k allows -- def_next[s] >= 0 as a fill over [0, eot), the explicit edges in parallel
//            (target >= 0 sets the bit, -1 clears it), accept[s] for eot; the dead state allows eot alone.
//   ban    : the row's ban words |= ~allowed over [0, eot], a plain read-modify-write of the words wm_repeat_state has just
//            rebuilt -- one workgroup owns the row.  Words wholly above eot are not touched; bits above eot are not changed.
// A row on start -1 and a prompt position (k < 0) write nothing.
// The walk is sequential -- up to 447 dependent lookups by ONE lane -- and each lookup is a probe of the (state, token) hash
// the host built (WmCstDev::hash: one 8-byte load per probe, the table at most half full) beside the load of def_next[s], which
// does not depend on the probe.  Rebuilding instead of carrying a per-row state: as wm_repeat_state -- a re-parented beam row, a
// finished row, a ragged row or a replayed graph needs no case of its own, and the kernel is a function of (history, position).
#include "model.h"

namespace {
constexpr int kThreads = 256;

// grid: B rows.  Dynamic LDS (32-bit words): allow [ban_words] | g [n_ctx] | state [1]
__global__ __launch_bounds__(kThreads) void constraint_state_kernel(const int *__restrict__ seq, const int *__restrict__ pos_ptr, int B,
                                                                    int n_prompt, int n_ctx, WmCstDev cst, unsigned *__restrict__ ban,
                                                                    int ban_words, int *__restrict__ state_out) {
    extern __shared__ unsigned cs_smem[];
    unsigned *allow = cs_smem;
    int *g = (int *)(cs_smem + ban_words);
    int *st = g + n_ctx;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int start = cst.start[b];
    int k = *pos_ptr + 1 - n_prompt;   // generated tokens so far
    if (start < 0 || k < 0) return;    // an unconstrained row, a prompt position: nothing is written (the same for the whole workgroup)
    const WmCstPar par = *cst.par;
    const int S = par.n_states < WM_MAX_CST_STATES ? par.n_states : WM_MAX_CST_STATES;
    const int eot = par.eot;
    // (the host has checked all of this; a block that would leave the tables or the row's words writes nothing instead)
    if (start >= S || eot < 0 || eot >= ban_words * 32 || eot > (1 << WM_CST_TOK_BITS)) return;
    k = k > n_ctx - n_prompt ? n_ctx - n_prompt : k;
    for (int i = tid; i < k; i += kThreads) g[i] = seq[(long)(n_prompt + i) * B + b];
    __syncthreads();
    if (tid == 0) {
        const int2 *hash = (const int2 *)cst.hash;
        int s = start;
        for (int i = 0; i < k && s >= 0; ++i) {
            const int t = g[i];
            if (t < 0 || t >= eot) continue;   // transparent: timestamps, specials, the padding of a finished row
            const unsigned key = wm_cst_key(s, t);
            unsigned at = wm_cst_slot(key);
            int nx = cst.def_next[s];
            for (int probe = 0; probe < WM_CST_HASH_SLOTS; ++probe) {
                const int2 e = hash[at];
                if ((unsigned)e.x == key) { nx = e.y; break; }
                if (e.x == -1) break;
                at = (at + 1) & (WM_CST_HASH_SLOTS - 1);
            }
            s = nx >= 0 && nx < S ? nx : -1;
        }
        st[0] = s;
        if (state_out) state_out[b] = s;
    }
    __syncthreads();
    const int s = st[0];
    const int aw = (eot >> 5) + 1;   // the words that hold [0, eot]
    const unsigned fill = s >= 0 && cst.def_next[s] >= 0 ? ~0u : 0u;
    for (int w = tid; w < aw; w += kThreads) allow[w] = fill;
    __syncthreads();
    if (s >= 0) {
        int e0 = cst.edge_beg[s], e1 = cst.edge_beg[s + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > WM_MAX_CST_EDGES ? WM_MAX_CST_EDGES : e1;
        for (int e = e0 + tid; e < e1; e += kThreads) {
            const int t = cst.edge_tok[e];
            if (t < 0 || t >= eot) continue;
            if (cst.edge_next[e] >= 0)
                atomicOr(&allow[t >> 5], 1u << (t & 31));
            else
                atomicAnd(&allow[t >> 5], ~(1u << (t & 31)));
        }
    }
    __syncthreads();
    const bool acc = s < 0 || cst.accept[s] != 0;   // the dead state allows eot alone
    unsigned *bo = ban + (long)b * ban_words;
    for (int w = tid; w < aw; w += kThreads) {
        unsigned a = allow[w], in = ~0u;   // in: the ids of the word that lie in [0, eot]
        if (w == aw - 1) {
            const unsigned bit = 1u << (eot & 31);
            in = bit | (bit - 1u);
            a = (a & (bit - 1u)) | (acc ? bit : 0u);
        }
        const unsigned bw = ~a & in;
        if (bw) bo[w] = bo[w] | bw;
    }
}
}  // namespace

int wm_constraint_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmCstDev &cst,
                        unsigned *ban, int ban_words, int *state_out) {
    WM_REQUIRE(seq && pos_ptr && ban && cst.par && cst.edge_beg && cst.edge_tok && cst.edge_next && cst.def_next && cst.accept &&
                   cst.hash && cst.start,
               WM_ERR_INVALID, "constraint_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && n_prompt >= 0 && n_ctx >= 1 && n_prompt <= n_ctx && V >= 1 && ban_words >= 1 &&
                   (long)ban_words * 32 >= V,
               WM_ERR_INVALID, "constraint_state: bad shape (B %d, prompt %d of %d, V %d, %d words)", B, n_prompt, n_ctx, V, ban_words);
    const size_t lds = ((size_t)ban_words + n_ctx + 1) * 4;
    WM_REQUIRE(lds <= 64 * 1024, WM_ERR_INVALID, "constraint_state: a vocabulary of %d ids does not fit the bitmap's 64 KiB of LDS", V);
    WmProfScope ps(&ctx->prof, "constraint_state", ctx->stream);
    constraint_state_kernel<<<B, kThreads, lds, ctx->stream>>>(seq, pos_ptr, B, n_prompt, n_ctx, cst, ban, ban_words, state_out);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
