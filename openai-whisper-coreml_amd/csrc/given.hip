// given.hip -- given tokens (wm_set_given_tokens): a row decodes a text the caller already has and
// returns its log-probs.  One launch per position of a group with WmDecodeMode::given, LAST in front of the close -- behind
// wm_alternatives (which therefore lists what the model preferred) and wm_sample_truncate (a given row overrides a draw).
// One 16-wave workgroup per row; a row that is done, a prompt position and a row with gi >= lens return at once and write
// nothing.  For a given row:
//   * `forced` from the partials through dec_close.h, as sample_trunc_kernel and alternatives_kernel have it;
//   * row_list.h's admissibility test on the one id, and its value from the stored f32 row (penalised and biased);
//   * the hand-over of sample_trunc.hip with a kept set of one: only the given id is left in the row's per-tile keys, the
//     winner value of its tile and side is its value (or -inf where it is not admissible).  The log-sum-exp partials stay, so
//     argmax_embed_body and dec_close.h run unchanged and the log-prob is value - the row's own normaliser.
// The cases, through row_choose / row_logprob of the close (K = argmax_key(value or -inf, id) > 1; F = the row's `forced`):
//   text, not F           : tilemax = {K}, key_ts = {}        -> kts 0: not forced, key K, norm over text + timestamps
//   text, F               : the same keys.  Not admissible: value -inf, the close's norm is the finite one over text + timestamps
//                           instead of the timestamps' (row_choose cannot force a timestamp and keep a text id) -- -inf either way
//   timestamp, not F      : tilemax = {1 in tile 0}, key_ts = {K} -> key 1: text_best = lt.m, lse <= lt.m as before: not forced,
//                           the winner is max(K, 1) = K, norm over text + timestamps
//   timestamp, F          : tilemax = {}, key_ts = {K}        -> key 0: forced, key K, norm over the timestamps
//   timestamp rules off   : tilemax = {K}                     -> key K, norm over the allowed ids
// and an id that is not admissible differs from an admissible one in its value alone.  A row with nothing admissible at all has
// no normaliser: it is left to the close's existing path (the fallback token, -inf), as sample_trunc_kernel leaves it.
#include "dec_close.h"
#include "model.h"
#include "row_list.h"

namespace {

// row_list.h's test (row_list_local_best) for one id
__device__ __forceinline__ bool given_admissible(const RowAdmit &a, int n) {
    const bool in_text = !a.forced && n >= a.rng.x && n < a.rng.y, in_ts = n >= a.rng.z && n < a.rng.w;
    const unsigned w = (a.mrow ? a.mrow[n >> 5] : 0u) | (a.brow ? a.brow[n >> 5] : 0u);
    return n >= 0 && n < a.V && (in_text || in_ts) && !((w >> (n & 31)) & 1u);
}

__global__ __launch_bounds__(1024) void given_tokens_kernel(const float *__restrict__ logits, long ldo, int V, int n_tiles,
                                                            unsigned long long *__restrict__ tilemax, WmTsDev ts, WmXDev xd,
                                                            const unsigned *__restrict__ mask, int mask_words, int n_prompt,
                                                            const int *__restrict__ pos_ptr, const int *__restrict__ done,
                                                            const unsigned *__restrict__ ban, int ban_words,
                                                            const WmGivenPar *__restrict__ par) {
    __shared__ float seg_s[16][4];
    __shared__ unsigned long long red_s[16];
    __shared__ int forced_s, live_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *pos_ptr, gi = pos + 1 - n_prompt;
    const WmGivenPar gp = *par;
    // workgroup-uniform: a prompt position, a position past the table, a row that is done, a row that decodes freely from here
    if (gi < 0 || gi >= gp.stride || (done && done[b]) || gi >= gp.lens[b]) return;
    const int tok = gp.tok[(long)b * gp.stride + gi];
    if (tok < 0 || tok >= V) return;   // (the setter checked: never index with it)
    const long rb = (long)b * n_tiles;
    // `forced` (the sum rule) from the partials: sample_trunc_kernel's steps
    lse_row_segments(xd, rb, n_tiles, false, wave, 16, lane, seg_s);
    {
        unsigned long long key = 0ull;
        if (ts.rng) {   // (the best allowed text key: row_choose asks whether there is one)
            for (int t = threadIdx.x; t < n_tiles; t += 1024) {
                const unsigned long long k = tilemax[rb + t];
                key = k > key ? k : key;
            }
            key = key_max_xor<64>(key);
        }
        if (lane == 0) red_s[wave] = key;
    }
    __syncthreads();
    if (wave == 0) {
        Lse lt{-1e30f, 0.f}, la{-1e30f, 0.f};
        lse_row_total(seg_s, lane, lt, la);
        unsigned long long key = lane < 16 ? red_s[lane] : 0ull;
        key = __shfl(key_max_xor<16>(key), 0);
        const RowChoice ch = row_choose(ts, b, n_tiles, lane, key, lt.m);
        if (lane == 0) {
            forced_s = ch.forced ? 1 : 0;
            const float vmax = ch.forced ? ch.lts.m : fmaxf(lt.m, ch.lts.m);   // (lts: (-1e30, 0) without timestamp rules)
            live_s = vmax > -1e30f ? 1 : 0;
        }
    }
    __syncthreads();   // (every read of the row's keys above is behind this barrier: the rewrite below may begin)
    if (!live_s) return;   // nothing admissible: the close takes its existing path (uniform)
    const bool forced = forced_s != 0;
    RowAdmit adm;
    adm.V = V;
    adm.rng = make_int4(0, V, 0, 0);
    if (ts.rng) adm.rng = *(const int4 *)(ts.rng + b * 4);
    adm.forced = forced;
    adm.mrow = mask ? mask + (pos == n_prompt - 1 ? mask_words : 0) : nullptr;
    adm.brow = ban ? ban + (long)b * ban_words : nullptr;
    const float v = logits[(long)b * ldo + tok];
    const float val = (given_admissible(adm, tok) && v > -INFINITY) ? v : -INFINITY;   // (NaN: not admissible)
    const unsigned long long win = argmax_key(val, tok);
    // the hand-over (sample_trunc.hip): only the given id is left in the row's keys.  A timestamp given where the sum rule did not
    // force one leaves the smallest key in the text keys, so that row_choose still sees admissible text below it.
    const int wt = tok >> 4;
    const int side = (ts.rng && tok >= ts.ts_begin) ? 1 : 0;
    const int t_first = ts.ts_begin >> 4;
    for (int t = threadIdx.x; t < n_tiles; t += 1024) {
        tilemax[rb + t] = (side == 0 && t == wt) ? win : ((side == 1 && !forced && t == 0) ? 1ull : 0ull);
        if (ts.rng && t >= t_first) ts.key_ts[rb + t] = (side == 1 && t == wt) ? win : 0ull;
    }
    if (threadIdx.x == 0) xd.win[(rb + wt) * 2 + side] = val;
}

}  // namespace

int wm_given_tokens(wm_ctx *ctx, const float *logits, long ldo, int n_vocab, unsigned long long *tilemax, int rows, const WmTsDev &ts,
                    const WmXDev &xd, const unsigned *mask, int mask_words, int n_prompt, const int *pos_ptr, const WmStopDev &stop,
                    const unsigned *ban, int ban_words, const WmGivenPar *par) {
    WmProfScope ps(&ctx->prof, "given_tokens", ctx->stream);
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && logits && tilemax && xd.par && xd.txt && xd.win && par && pos_ptr, WM_ERR_INVALID,
               "given_tokens: bad group");
    WM_REQUIRE(n_vocab >= 1 && ldo >= n_vocab, WM_ERR_INVALID, "given_tokens: %d ids in rows of %ld", n_vocab, ldo);
    WM_REQUIRE(!mask || (long)mask_words * 32 >= n_vocab, WM_ERR_INVALID, "given_tokens: %d mask words do not cover %d ids", mask_words,
               n_vocab);
    WM_REQUIRE(!ban || (long)ban_words * 32 >= n_vocab, WM_ERR_INVALID, "given_tokens: %d ban words do not cover %d ids", ban_words, n_vocab);
    WM_REQUIRE(!ts.rng || (ts.key_ts && ts.lse && ts.ts_begin >= 0), WM_ERR_INVALID, "given_tokens: incomplete timestamp-rule state");
    given_tokens_kernel<<<rows, 1024, 0, ctx->stream>>>(logits, ldo, n_vocab, (n_vocab + 15) / 16, tilemax, ts, xd, mask, mask_words,
                                                        n_prompt, pos_ptr, stop.done, ban, ban_words, par);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
