// alternatives.hip -- top-n alternatives and entropy per generated token (wm_request_alternatives): one
// launch per position of a group with WmDecodeMode::alt, between the DE_LOGITS_X* product (which stored the f32 row, penalised
// and biased, and left the per-tile partials) and the close -- in a group with the sampling rules BEFORE wm_sample_truncate,
// which rewrites the per-tile keys.  One 16-wave workgroup per row:
//   * `forced` and the normaliser from the partials through dec_close.h, exactly as beam_topk_kernel has them; the
//     admissibility test and the descending-key list scan are row_list.h's, which that kernel calls too;
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
    const long rb = (long)b * n_tiles;
    lse_row_segments(xd, rb, n_tiles, false, wave, 16, lane, seg_s);
    {   // the best allowed text key of the row (decides the sum rule with the timestamps' log-sum-exp)
        unsigned long long key = 0ull;
        for (int t = threadIdx.x; t < n_tiles; t += 1024) {
            const unsigned long long k = tilemax[rb + t];
            key = k > key ? k : key;
        }
        key = key_max_xor<64>(key);
        if (lane == 0) red_s[0][wave] = key;
    }
    __syncthreads();
    if (wave == 0) {
        Lse lt{-1e30f, 0.f}, la{-1e30f, 0.f};
        lse_row_total(seg_s, lane, lt, la);
        unsigned long long key = lane < 16 ? red_s[0][lane] : 0ull;
        key = __shfl(key_max_xor<16>(key), 0);
        const RowChoice ch = row_choose(ts, b, n_tiles, lane, key, lt.m);   // (for `forced` and the normaliser)
        const float norm = row_log_norm(ts, ch, lt);
        if (lane == 0) {
            norm_s = norm;
            forced_s = ch.forced ? 1 : 0;
        }
    }
    __syncthreads();
    const float norm = norm_s;
    RowAdmit adm;
    adm.V = V;
    adm.rng = make_int4(0, V, 0, 0);
    if (ts.rng) adm.rng = *(const int4 *)(ts.rng + b * 4);
    adm.forced = forced_s != 0;
    adm.mrow = mask ? mask + (pos == n_prompt - 1 ? mask_words : 0) : nullptr;
    adm.brow = ban ? ban + (long)b * ban_words : nullptr;
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

int wm_alternatives(wm_ctx *ctx, const float *logits, long ldo, int n_vocab, const unsigned long long *tilemax, int rows,
                    const WmTsDev &ts, const WmXDev &xd, const unsigned *mask, int mask_words, int n_prompt, const int *pos_ptr,
                    const WmStopDev &stop, const unsigned *ban, int ban_words, const WmAltPar *par) {
    WmProfScope ps(&ctx->prof, "alternatives", ctx->stream);
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && logits && tilemax && xd.par && xd.txt && par && pos_ptr, WM_ERR_INVALID,
               "alternatives: bad group");
    WM_REQUIRE(n_vocab >= 1 && ldo >= n_vocab, WM_ERR_INVALID, "alternatives: %d ids in rows of %ld", n_vocab, ldo);
    WM_REQUIRE(!mask || (long)mask_words * 32 >= n_vocab, WM_ERR_INVALID, "alternatives: %d mask words do not cover %d ids", mask_words,
               n_vocab);
    WM_REQUIRE(!ban || (long)ban_words * 32 >= n_vocab, WM_ERR_INVALID, "alternatives: %d ban words do not cover %d ids", ban_words, n_vocab);
    WM_REQUIRE(!ts.rng || (ts.key_ts && ts.lse && ts.ts_begin >= 0), WM_ERR_INVALID, "alternatives: incomplete timestamp-rule state");
    alternatives_kernel<<<rows, 1024, 0, ctx->stream>>>(logits, ldo, n_vocab, (n_vocab + 15) / 16, tilemax, ts, xd, mask, mask_words,
                                                        n_prompt, pos_ptr, stop.done, ban, ban_words, par);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
