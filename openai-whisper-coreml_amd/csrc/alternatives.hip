// alternatives.hip -- top-n alternatives and entropy per generated token (wm_request_alternatives): one
// launch per position of a group with WmDecodeMode::alt, between the DE_LOGITS_X* product (which stored the f32 row, penalised
// and biased, and left the per-tile partials) and the close -- in a group with the sampling rules BEFORE wm_sample_truncate,
// which rewrites the per-tile keys.  One 16-wave workgroup per row:
//   * `forced` and the normaliser from the partials: stored_row.h's prologue, and its admissible set; the descending-key list
//     scan is row_list.h's -- beam_topk_kernel calls all three too;
//   * the entropy -sum p log p over the admissible ids shares the scan's first read of the row: thread t adds its ids
//     ascending, then one fixed tree (a butterfly per wave, a butterfly over the 16 wave sums).  f32 adds commute, so every
//     lane of a butterfly holds the same bits, and a row's bits depend on the row alone.
// The kernel reads the partials and writes its own buffers only: the close that follows sees what it would have seen.
#include "dec_close.h"
#include "model.h"
#include "row_list.h"

namespace {

__global__ __launch_bounds__(1024) void alternatives_kernel(const float *__restrict__ logits, long ldo, int V, int n_tiles,
                                                            const unsigned long long *__restrict__ tilemax, WmTsDev ts, WmXDev xd,
                                                            const unsigned *__restrict__ mask, int mask_words, int n_prompt,
                                                            const int *__restrict__ pos_ptr, const int *__restrict__ done,
                                                            const unsigned *__restrict__ ban, int ban_words,
                                                            const WmAltPar *__restrict__ par) {
    __shared__ float seg_s[16][4];
    __shared__ unsigned long long red_s[2][16];
    __shared__ float norm_s, ent_s[16];
    __shared__ int forced_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *pos_ptr, gi = pos + 1 - n_prompt;
    const WmAltPar ap = *par;
    // workgroup-uniform: a prompt position, a position past the buffers, a row that is done (a window that has left: its rows
    // are done) -- the buffers keep the pads of the prefill
    if (gi < 0 || gi >= ap.max_new || ap.n < 1 || ap.n > WM_MAX_ALTERNATIVES || (done && done[b])) return;
    // `forced` and the normaliser from the partials (the list scan below picks: ch.key is not used)
    stored_row_prologue(ts, xd, tilemax, b, n_tiles, false, seg_s, red_s[0], [&](const RowChoice &ch, Lse lt, Lse) {
        const float norm = row_log_norm(ts, ch, lt);
        if (lane == 0) {
            norm_s = norm;
            forced_s = ch.forced ? 1 : 0;
        }
    });
    const float norm = norm_s;
    const RowAdmit adm = row_admit_set(V, ts, mask, mask_words, ban, ban_words, b, pos, n_prompt, forced_s != 0);
    const long at = (long)gi * gridDim.x + b;   // [gi][row]
    int *tok = ap.tok + at * ap.n;
    float *lps = ap.lp + at * ap.n;
    float h = 0.f;   // this thread's share of -sum p log p, its ids ascending
    const int count = row_list_scan(logits + (long)b * ldo, adm, ap.n, norm, red_s,
                                    [&](int, float v) {
                                        const float lp = v - norm;
                                        if (lp > -INFINITY) h = __fsub_rn(h, __fmul_rn(__expf(lp), lp));   // (-inf, NaN: not in A)
                                    },
                                    [&](int r, unsigned long long key, float lp) {
                                        tok[r] = argmax_key_index(key);
                                        lps[r] = lp;
                                    });
    if ((int)threadIdx.x >= count && (int)threadIdx.x < ap.n) {   // entries past the count are pads
        tok[threadIdx.x] = -1;
        lps[threadIdx.x] = 0.f;
    }
    if (threadIdx.x == 0 && ap.cnt) ap.cnt[at] = count;
    if (!ap.ent) return;   // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h = __fadd_rn(h, __shfl_xor(h, o));
    if (lane == 0) ent_s[wave] = h;
    __syncthreads();
    if (wave == 0) {
        h = lane < 16 ? ent_s[lane] : 0.f;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) h = __fadd_rn(h, __shfl_xor(h, o));
        if (lane == 0) ap.ent[at] = h;
    }
}

}  // namespace

int wm_alternatives(wm_ctx *ctx, const WmStoredRows &r, const WmAltPar *par) {
    WmProfScope ps(&ctx->prof, "alternatives", ctx->stream);
    WM_TRY(wm_stored_rows_check(r, "alternatives", false));
    WM_REQUIRE(par, WM_ERR_INVALID, "alternatives: no parameters");
    alternatives_kernel<<<r.rows, 1024, 0, ctx->stream>>>(r.logits, r.ldo, r.n_vocab, (r.n_vocab + 15) / 16, r.tilemax, r.ts, r.xd, r.mask,
                                                          r.mask_words, r.n_prompt, r.pos_ptr, r.stop.done, r.ban, r.ban_words, par);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
