// given.hip -- given tokens (wm_set_given_tokens): a row decodes a text the caller already has and
// returns its log-probs.  One launch per position of a group with WmDecodeMode::given, LAST in front of the close -- behind
// wm_alternatives (which therefore lists what the model preferred) and wm_sample_truncate (a given row overrides a draw).
// One 16-wave workgroup per row; a row that is done, a prompt position and a row with gi >= lens return at once and write
// nothing.  For a given row, every step is stored_row.h's:
//   * `forced` from the partials: stored_row_prologue;
//   * the admissibility test on the one id (row_admit_set, row_admits), and its value from the stored f32 row (penalised and
//     biased);
//   * the hand-over (row_hand_over) with a kept set of one: only the given id is left in the row's per-tile keys, the winner
//     value of its tile and side is its value (or -inf where it is not admissible).  The log-sum-exp partials stay, so
//     argmax_embed_body and dec_close.h run unchanged and the log-prob is value - the row's own normaliser.
// The cases through row_choose / row_logprob of the close are the table at row_hand_over.  A row with nothing admissible at all
// has no normaliser: it is left to the close's existing path (the fallback token, -inf), as sample_trunc_kernel leaves it.
#include "dec_close.h"
#include "model.h"
#include "stored_row.h"

namespace {

__global__ __launch_bounds__(1024) void given_tokens_kernel(const float *__restrict__ logits, long ldo, int V, int n_tiles,
                                                            unsigned long long *__restrict__ tilemax, WmTsDev ts, WmXDev xd,
                                                            const unsigned *__restrict__ mask, int mask_words, int n_prompt,
                                                            const int *__restrict__ pos_ptr, const int *__restrict__ done,
                                                            const unsigned *__restrict__ ban, int ban_words,
                                                            const WmGivenPar *__restrict__ par) {
    __shared__ float seg_s[16][4];
    __shared__ unsigned long long red_s[16];
    __shared__ int forced_s, live_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int pos = *pos_ptr, gi = pos + 1 - n_prompt;
    const WmGivenPar gp = *par;
    // workgroup-uniform: a prompt position, a position past the table, a row that is done, a row that decodes freely from here
    if (gi < 0 || gi >= gp.stride || (done && done[b]) || gi >= gp.lens[b]) return;
    const int tok = gp.tok[(long)b * gp.stride + gi];
    if (tok < 0 || tok >= V) return;   // (the setter checked: never index with it)
    const long rb = (long)b * n_tiles;
    stored_row_prologue(ts, xd, tilemax, b, n_tiles, false, seg_s, red_s, [&](const RowChoice &ch, Lse lt, Lse) {
        if (lane == 0) {
            forced_s = ch.forced ? 1 : 0;
            live_s = row_best_value(ch, lt) > -1e30f ? 1 : 0;
        }
    });   // (every read of the row's keys is behind the prologue's last barrier: the rewrite below may begin)
    if (!live_s) return;   // nothing admissible: the close takes its existing path (uniform)
    const bool forced = forced_s != 0;
    const RowAdmit adm = row_admit_set(V, ts, mask, mask_words, ban, ban_words, b, pos, n_prompt, forced);
    const float v = logits[(long)b * ldo + tok];
    const float val = (row_admits(adm, tok) && v > -INFINITY) ? v : -INFINITY;   // (NaN: not admissible)
    row_hand_over(ts, tilemax, rb, n_tiles, forced, argmax_key(val, tok), threadIdx.x, 1024);
    if (threadIdx.x == 0) xd.win[row_win_slot(ts, rb, tok)] = val;
}

}  // namespace

int wm_given_tokens(wm_ctx *ctx, const WmStoredRows &r, const WmGivenPar *par) {
    WmProfScope ps(&ctx->prof, "given_tokens", ctx->stream);
    WM_TRY(wm_stored_rows_check(r, "given_tokens", true));
    WM_REQUIRE(par, WM_ERR_INVALID, "given_tokens: no table");
    given_tokens_kernel<<<r.rows, 1024, 0, ctx->stream>>>(r.logits, r.ldo, r.n_vocab, (r.n_vocab + 15) / 16, r.tilemax, r.ts, r.xd, r.mask,
                                                          r.mask_words, r.n_prompt, r.pos_ptr, r.stop.done, r.ban, r.ban_words, par);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
