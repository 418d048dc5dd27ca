// beam.hip -- the close of a generating position of a beam group (wm_transcribe_mel_beam): three
// launches behind the decode step's DE_LOGITS_X product (which leaves the f32 logits and the filtered per-tile partials):
//   * beam_topk_kernel   : per row, the log-sum-exp of the admissible ids and its N + 1 best tokens;
//   * beam_select_kernel : per window, the selection rule of beam.h, the finished records, the rows' new state, the
//                          embedding of the next position, the live list and the position advance; in an aligned group
//                          (WmBeamDev::anc) also the ancestry record wm_beam_ancestry walks;
//   * beam_reorder_kernel: the self-attention K/V cache and the rows' histories gathered by source beam, in place.
// A beam of width 1 must reproduce the greedy decode BIT FOR BIT (tokens, log-probs), so a row's close here is the
// arithmetic of dec_kernels.hip's argmax_embed_body in its summation orders (16 fixed tile segments, one wave per row for
// the merges and the embedding): both call the same functions of dec_close.h -- lse_row_segments, lse_row_total,
// row_choose (with ts_row_merge inside), row_log_norm, row_no_speech, ts_advance, embed_row, live_list_rebuild; the list
// kernel's prologue and admissible set are stored_row.h's, shared with the other kernels on a stored row -- and
// tests/test_beam_gpu.py (end to end) and tests/test_close_shared_gpu.py (on one step's partials) hold the closes to equal bits.
#include "beam.h"
#include "dec_close.h"
#include "model.h"
#include "row_list.h"

namespace {

// ------------------------------------------------------------------ per-row list ------------------------------------
// One 16-wave workgroup per row.  The reductions are maxima (any order, same bits) except the log-sum-exp, which follows
// the fixed orders of dec_close.h: a row's list does not depend on the group's shape.
__global__ __launch_bounds__(1024) void beam_topk_kernel(const float *__restrict__ logits, long ldo, int V, int n_tiles,
                                                         const unsigned long long *__restrict__ tilemax, WmTsDev ts, WmXDev xd,
                                                         const unsigned *__restrict__ mask, int mask_words, int n_prompt,
                                                         const int *__restrict__ pos_ptr, WmBeamDev bm,
                                                         const unsigned *__restrict__ ban, int ban_words) {
    __shared__ float seg_s[16][4];
    __shared__ unsigned long long red_s[2][16];
    __shared__ float norm_s;
    __shared__ int forced_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int pos = *pos_ptr, gi = pos + 1 - n_prompt;
    const int K = bm.N + 1;
    const float my_sum = bm.sum[b];
    float *tr = bm.trace ? bm.trace + ((long)gi * gridDim.x + b) * WM_BEAM_TRACE : nullptr;
    if (bm.wdone[b / bm.N] || my_sum == -INFINITY) {   // workgroup-uniform: the window has left, or a dead beam
        if (threadIdx.x == 0) {
            bm.list_n[b] = 0;
            if (tr) { tr[0] = __int_as_float(0); tr[1] = my_sum; }
        }
        return;
    }
    const bool sot = pos == xd.par->sot_pos;
    // `forced` and the normaliser from the partials (the list scan below picks: ch.key is not used)
    stored_row_prologue(ts, xd, tilemax, b, n_tiles, sot, seg_s, red_s[0], [&](const RowChoice &ch, Lse lt, Lse la) {
        const float norm = row_log_norm(ts, ch, lt);
        if (lane == 0) {
            norm_s = norm;
            forced_s = ch.forced ? 1 : 0;
            if (sot) xd.nospeech[b] = row_no_speech(xd, b, la);
        }
    });
    const float norm = norm_s;
    // the row's N + 1 best admissible ids in descending key order: the list scan of row_list.h
    const RowAdmit adm = row_admit_set(V, ts, mask, mask_words, ban, ban_words, b, pos, n_prompt, forced_s != 0);
    const int count = row_list_scan(logits + (long)b * ldo, adm, K, norm, red_s, [](int, float) {},
                                    [&](int r, unsigned long long key, float lp) {
        bm.list_tok[b * WM_BEAM_LIST + r] = argmax_key_index(key);
        bm.list_lp[b * WM_BEAM_LIST + r] = lp;
        if (tr) { tr[2 + r] = __int_as_float(argmax_key_index(key)); tr[2 + WM_BEAM_LIST + r] = lp; }
    });
    if (threadIdx.x == 0) {
        bm.list_n[b] = count;
        if (tr) { tr[0] = __int_as_float(count); tr[1] = my_sum; }
    }
}

// ------------------------------------------------------------------ per-window step ---------------------------------
// ONE workgroup: wave v takes windows v, v + 16, ...; nothing is handed between workgroups.
__global__ __launch_bounds__(1024) void beam_select_kernel(int B, int *__restrict__ seq, int *__restrict__ pos_ptr, int n_prompt,
                                                           const bf16_t *__restrict__ emb, const float *__restrict__ pemb, int d,
                                                           float *__restrict__ x, bf16_t *__restrict__ xb,
                                                           float *__restrict__ stats_out, float *__restrict__ mean_buf, WmTsDev ts,
                                                           WmStopDev stop, WmXDev xd, const int *__restrict__ off, WmBeamDev bm) {
    __shared__ WmBeamStep step_s[16];
    __shared__ float sum_s[16][WM_MAX_BEAM], lp_s[16][WM_MAX_BEAM * WM_BEAM_LIST];
    __shared__ int ln_s[16][WM_MAX_BEAM], tok_s[16][WM_MAX_BEAM * WM_BEAM_LIST];
    __shared__ __align__(16) int hist_s[16][WM_MAX_BEAM][4];
    __shared__ int done_s[WM_DEC_MAXB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *pos_ptr, gi = pos + 1 - n_prompt, N = bm.N, C = B / N;
    const WmBeamPar par = *bm.par;
    for (int w = wave; w < C; w += 16) {   // wave-uniform
        const int row0 = w * N;
        const bool was_done = bm.wdone[w] != 0;
        WmBeamStep &st = step_s[wave];
        if (was_done) {   // the window has left: padding, nothing moves
            if (lane < N) {
                seq[(pos + 1) * B + row0 + lane] = par.pad;
                xd.logprob[(long)gi * B + row0 + lane] = 0.f;
                bm.src[row0 + lane] = lane;
                if (bm.anc) bm.anc[gi * B + row0 + lane] = lane;
                done_s[row0 + lane] = 1;
                st.tok[lane] = par.pad;
            }
        } else {
            if (lane < N) {
                sum_s[wave][lane] = bm.sum[row0 + lane];
                ln_s[wave][lane] = bm.list_n[row0 + lane];
                if (ts.rng) *(int4 *)hist_s[wave][lane] = *(const int4 *)(ts.hist + (row0 + lane) * 4);
            }
            for (int e = lane; e < N * WM_BEAM_LIST; e += 64) {
                tok_s[wave][e] = bm.list_tok[row0 * WM_BEAM_LIST + e];
                lp_s[wave][e] = bm.list_lp[row0 * WM_BEAM_LIST + e];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nfin0 = bm.fin_n[w];
            if (lane == 0)
                wm_beam_select(N, gi == 0 ? 1 : N, par.eot, par.pad, par.max_cand - nfin0, sum_s[wave], ln_s[wave], tok_s[wave],
                               lp_s[wave], &st);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // newly finished hypotheses: the source beam's history, then eot
            for (int f = 0; f < st.n_fin; ++f) {
                const int slot = nfin0 + f, srow = row0 + st.fin_src[f];
                const long base = ((long)w * WM_MAX_BEAM_HYPS + slot) * bm.n_ctx;
                for (int i = lane; i < gi; i += 64) {
                    bm.fin_tok[base + i] = seq[(n_prompt + i) * B + srow];
                    bm.fin_lp[base + i] = xd.logprob[(long)i * B + srow];
                }
                if (lane == 0) {
                    bm.fin_tok[base + gi] = par.eot;
                    bm.fin_lp[base + gi] = st.fin_lp[f];
                    bm.fin_len[w * WM_MAX_BEAM_HYPS + slot] = gi + 1;
                    bm.fin_sum[w * WM_MAX_BEAM_HYPS + slot] = st.fin_sum[f];
                    if (bm.fin_src) bm.fin_src[w * WM_MAX_BEAM_HYPS + slot] = st.fin_src[f];
                }
            }
            const int nfin = nfin0 + st.n_fin;
            const bool leaves = nfin >= par.max_cand || gi + 1 >= bm.budget[w];
            if (lane < N) {
                const int row = row0 + lane, tok = st.tok[lane];
                seq[(pos + 1) * B + row] = tok;
                xd.logprob[(long)gi * B + row] = st.lp[lane];
                bm.sum[row] = st.sum[lane];
                bm.src[row] = st.src[lane];
                if (bm.anc) bm.anc[gi * B + row] = st.src[lane];
                if (ts.rng) {   // the timestamp-rule state follows the source beam
                    __align__(16) int hs[4];
                    *(int4 *)hs = *(const int4 *)hist_s[wave][st.src[lane]];
                    const int4 rng = ts_advance(ts, hs, tok);
                    *(int4 *)(ts.hist + row * 4) = *(const int4 *)hs;
                    *(int4 *)(ts.rng + row * 4) = rng;
                }
                done_s[row] = (leaves || st.sum[lane] == -INFINITY) ? 1 : 0;
            }
            if (lane == 0) {
                bm.fin_n[w] = nfin;
                bm.wdone[w] = leaves ? 1 : 0;
                bm.wsteps[w] = gi + 1;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // st.tok: written by the lanes above, read by every lane
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (pos + 1 < bm.n_ctx) {
            for (int k = 0; k < N; ++k) {
                const int row = row0 + k;
                // a ragged group (off != null): the row's prompt starts at position off[row], its positional row counts from there
                const int prow = off ? max(pos + 1 - off[row], 0) : pos + 1;
                embed_row((long)st.tok[k], prow, row, lane, emb, pemb, d, x, xb, stats_out, mean_buf);
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        if (stop.done) {   // early stop: the flags and the compact list of live rows the attention kernels walk
            live_list_rebuild(stop, B, lane, [&](int b) {
                const bool live = done_s[b] == 0;
                stop.done[b] = live ? 0 : 1;
                return live;
            });
        }
        if (lane == 0) *pos_ptr = pos + 1;
    }
}

// ------------------------------------------------------------------ re-parenting ------------------------------------
// grid (H, L2 + 1, windows).  y < L2: the 128-byte rows [0, p] of one (layer, K or V, head) of a window's N beams, 16 bytes per
// thread: a thread reads its unit of every source row before it writes it to any row, and no other thread touches that
// unit, so the gather is safe in place.  y == L2 (x == 0): the token and log-prob histories, one position per thread.
// p = *pos_ptr - 1, the position wm_beam_select_step has just closed.
template <int N>
__global__ __launch_bounds__(256) void beam_reorder_kernel(bf16_t *__restrict__ skv, int L2, int rows, int H, int T,
                                                           const int *__restrict__ pos_ptr, int n_prompt, int *__restrict__ seq,
                                                           float *__restrict__ logprob, WmBeamDev bm) {
    const int w = blockIdx.z, row0 = w * N;
    int s[N];
    bool same = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        s[k] = bm.src[row0 + k];
        same = same && s[k] == k;
    }
    if (same) return;   // (a window that left earlier, a step that kept every beam in place: nothing moves)
    const int p = *pos_ptr - 1, gi = p + 1 - n_prompt;
    if ((int)blockIdx.y == L2) {
        if (blockIdx.x != 0) return;
        for (int i = threadIdx.x; i < gi; i += 256) {   // (index gi is the new token, written in the new order already)
            int tk[N];
            float lp[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                tk[k] = seq[(n_prompt + i) * rows + row0 + s[k]];
                lp[k] = logprob[(long)i * rows + row0 + s[k]];
            }
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (s[k] == k) continue;
                seq[(n_prompt + i) * rows + row0 + k] = tk[k];
                logprob[(long)i * rows + row0 + k] = lp[k];
            }
        }
        return;
    }
    if (bm.wdone[w]) return;   // the window has just left: its caches are not read again
    const size_t slice = (size_t)T * 64;   // elements of one (row, head)
    uint4 *base = (uint4 *)(skv + (((size_t)blockIdx.y * rows + row0) * H + blockIdx.x) * slice);
    const size_t row_u = (size_t)H * slice / 8;   // 16-byte units between consecutive rows
    const int n_u = (p + 1) * 8;
    for (int q = threadIdx.x; q < n_u; q += 256) {
        uint4 v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (s[k] != k) v[k] = base[(size_t)s[k] * row_u + q];
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (s[k] != k) base[(size_t)k * row_u + q] = v[k];
    }
}

}  // namespace

int wm_beam_topk(wm_ctx *ctx, const WmStoredRows &r, const WmBeamDev &bm) {
    WmProfScope ps(&ctx->prof, "beam_topk", ctx->stream);
    WM_TRY(wm_stored_rows_check(r, "beam_topk", false));
    WM_REQUIRE(bm.N >= 1 && bm.N <= WM_MAX_BEAM && r.rows % bm.N == 0, WM_ERR_INVALID, "beam_topk: bad group");
    beam_topk_kernel<<<r.rows, 1024, 0, ctx->stream>>>(r.logits, r.ldo, r.n_vocab, (r.n_vocab + 15) / 16, r.tilemax, r.ts, r.xd, r.mask,
                                                       r.mask_words, r.n_prompt, r.pos_ptr, bm, r.ban, r.ban_words);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_beam_select_step(wm_ctx *ctx, int rows, int *seq, int *pos_ptr, int n_prompt, const WmEmbedDev &e, const WmTsDev &ts,
                        const WmStopDev &stop, const WmXDev &xd, const int *off, const WmBeamDev &bm) {
    WmProfScope ps(&ctx->prof, "beam_select", ctx->stream);
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && bm.N >= 1 && bm.N <= WM_MAX_BEAM && rows % bm.N == 0 && xd.par, WM_ERR_INVALID,
               "beam_select: bad group");
    beam_select_kernel<<<1, 1024, 0, ctx->stream>>>(rows, seq, pos_ptr, n_prompt, e.emb, e.pemb, e.d, e.x, e.xb, e.stats_out, e.mean_buf,
                                                    ts, stop, xd, off, bm);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_beam_reorder(wm_ctx *ctx, bf16_t *skv, int L2, int rows, int H, int T, const int *pos_ptr, int n_prompt, int *seq,
                    float *logprob, const WmBeamDev &bm) {
    WmProfScope ps(&ctx->prof, "beam_reorder", ctx->stream);
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && bm.N >= 1 && bm.N <= WM_MAX_BEAM && rows % bm.N == 0, WM_ERR_INVALID,
               "beam_reorder: bad group");
    if (bm.N == 1) return WM_OK;   // one beam per window: its source is itself
    const dim3 grid(H, L2 + 1, rows / bm.N);
#define WM_BEAM_REORDER_CASE(n)                                                                                            \
    case n:                                                                                                                \
        beam_reorder_kernel<n><<<grid, 256, 0, ctx->stream>>>(skv, L2, rows, H, T, pos_ptr, n_prompt, seq, logprob, bm);   \
        break;
    switch (bm.N) {
        WM_BEAM_REORDER_CASE(2) WM_BEAM_REORDER_CASE(3) WM_BEAM_REORDER_CASE(4) WM_BEAM_REORDER_CASE(5)
        WM_BEAM_REORDER_CASE(6) WM_BEAM_REORDER_CASE(7) WM_BEAM_REORDER_CASE(8)
    }
#undef WM_BEAM_REORDER_CASE
    WM_HIP(hipGetLastError());
    return WM_OK;
}
