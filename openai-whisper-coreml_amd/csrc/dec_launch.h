// dec_launch.h -- the launch shapes of the decode step as pure functions (dec_launch.cpp).
//
// Every decode launcher of dec_kernels.hip asks a plan function here for its kernel instantiation, grid, block, dynamic LDS,
// warm-up tiles and packed scalar arguments, then launches exactly that.  A plan is integer arithmetic on the launch's
// geometry, the CUs of the lane and the tuning knobs: plain C++, no HIP headers, no context, no global state -- so
// tests/test_dec_launch_cpu.py pins every rule on the CPU (wmdbg_dec_attn_plan / wmdbg_dec_gemv_plan) against the
// restatement in tests/dec_launch_ref.py.  A new launch shape goes HERE, with a line in that test.
#pragma once
#include <stdint.h>

#include "wm_tuning.h"

constexpr int WM_DEC_MAXB = 128;   // decode group: up to eight batch blocks of 16 rows (the MFMA M dimension)
constexpr int WM_ATT_MAXK = 1536;  // keys per (sequence, head) pair the attention kernels are built for

// DE_LOGITS_X: DE_LOGITS plus the WmXDev partials (text (max, sum exp), winners' raw logits, the unfiltered partial at
// the <|startoftranscript|> position) and Gumbel-perturbed keys when sampling -- its own instantiations, so the plain
// greedy logits kernel does none of it
// DE_LOGITS_XR: DE_LOGITS_X with the repetition rules (WmRepDev): the same body, the row's penalty and ban words applied to
// the logit first -- again its own instantiations, so DE_LOGITS_X stays instruction for instruction what it was
// DE_QKV_P: DE_QKV of a panel step (DecGemvArgs::panel = w): k / v of row r go to cache entry r / w at position *pos_ptr + r % w --
// its own instantiations, so DE_QKV stays instruction for instruction what it was
// DE_LOGITS_XB: DE_LOGITS_XR with the sequence bias (WmSbDev): the same body, the row's bias total added
// to the logit behind the penalty -- its own instantiations once more, so DE_LOGITS_X and DE_LOGITS_XR stay what they were
enum DecEpi { DE_QKV = 0, DE_Q = 1, DE_RESID = 2, DE_GELU = 3, DE_LOGITS = 4, DE_LOGITS_X = 5, DE_LOGITS_XR = 6, DE_QKV_P = 7, DE_LOGITS_XB = 8 };
// the extended-decode epilogues (DE_LOGITS_XR = DE_LOGITS_X + the repetition rules, DE_LOGITS_XB = DE_LOGITS_XR + the sequence
// bias), the ones that read the repetition bitmaps, and every logits epilogue
constexpr bool de_is_x(int epi) { return epi == DE_LOGITS_X || epi == DE_LOGITS_XR || epi == DE_LOGITS_XB; }
constexpr bool de_has_rep(int epi) { return epi == DE_LOGITS_XR || epi == DE_LOGITS_XB; }
constexpr bool de_is_logits(int epi) { return epi == DE_LOGITS || de_is_x(epi); }
constexpr bool de_is_qkv(int epi) { return epi == DE_QKV || epi == DE_QKV_P; }

// ---------------------------------------------------------------- packed kernel arguments ----
// The attention kernels take their hot scalars as three packed words (fewer preloaded SGPRs).  One pack / unpack pair per
// kernel family; pack returns false when a field does not fit its bits.  (The kernels take the words apart with their own
// shifts -- device code is kept instruction for instruction -- and name the helper that packs.)
struct DecAttnWords { unsigned a, b, c; };
// every family's packB: T_stride | n_keys << 16
bool wm_pack_attn_keys(int T_stride, int n_keys, unsigned *b);
void wm_unpack_attn_keys(unsigned b, int *T_stride, int *n_keys);
// dec_rows_attn_kernel / dec_xrows_attn_kernel: packA = H | nsplit << 8 | flat_wpw << 16, packC = n_bh | n_wg << 16
bool wm_pack_attn_rows(int H, int nsplit, int flat_wpw, int n_bh, int n_wg, unsigned *a, unsigned *c);
void wm_unpack_attn_rows(unsigned a, unsigned c, int *H, int *nsplit, int *flat_wpw, int *n_bh, int *n_wg);
// dec_xcand_attn_kernel: packA = H | flat_wpw << 16, packC = C | n_wg << 16
bool wm_pack_attn_cand(int H, int flat_wpw, int C, int n_wg, unsigned *a, unsigned *c);
void wm_unpack_attn_cand(unsigned a, unsigned c, int *H, int *flat_wpw, int *C, int *n_wg);
// dec_xattn_fq_kernel: packA = H | B << 8 (no packC)
bool wm_pack_attn_fq(int H, int B, unsigned *a);
void wm_unpack_attn_fq(unsigned a, int *H, int *B);

// ---------------------------------------------------------------- shared rules, each stated once ----
// L2 warm-up of the NEXT launch's weight matrix by extra workgroups of the current one: a latency lever for a decode
// group of one batch block (the next GEMV finds its weights in L2: ~1 us off a 4-5 us launch).  Larger groups are
// throughput-bound and run beside other groups; there the extra workgroups only take slots and bandwidth (measured,
// 3 groups of 56 chunks: 1978 -> 2007 audio-s/s without).
// rows: the rows of the decode group; has_pf / pf_rows / pf_k: the warm-up triple; compute_grid: the workgroups in front of
// the warm-up ones -- a multiple of 8, so that tile t lands on the XCD whose workgroup t consumes it.  Returns the tiles
// (0: no warm-up), *tile_bytes = the bytes of one 16-row tile of that matrix (0 without warm-up).
// How the call sites differ (each keeps what it did before the rule was written once):
//   * the cross-attention adds "not a split launch" (nsplit == 1): the caller passes has_pf = false otherwise;
//   * the candidate launch decided the tiles first and dropped them when its grid was no multiple of 8: the same condition;
//   * the fused-query launch never tested its grid: it is 8 * ceil(pairs / 8), a multiple of 8 by construction;
//   * the GEMV adds 32 * (pf_head_major / B + 2) workgroups instead of `tiles` when the consumer is head-major.
int wm_dec_warm_tiles(int rows, bool has_pf, int pf_rows, int pf_k, int compute_grid, const WmTuning &t, long *tile_bytes);
// Persistent cross-attention workgroups: at most one per CU of the lane (or xattn_wgs), balanced -- every workgroup walks
// `rounds` (or rounds - 1) pairs; short_lived (the chip is shared with other decode groups): one workgroup per pair.
int wm_dec_persistent_wgs(int pairs, int n_cus, bool short_lived, const WmTuning &t);
// The flat deal of a few pairs: (pair, stream) units dealt evenly over ~256 workgroups of *wpw <= wave_cap waves; *g = the
// workgroups.  wave_cap: 4 for dec_rows / dec_xrows (the DEEP kernel is built for <= 4 waves), 8 for dec_xcand.
void wm_dec_flat_deal(int pairs, int wave_cap, int *wpw, int *g);
// Workgroups per (sequence, head) pair of the cross-attention: 1 when the pairs alone fill the chip, else the stream
// set of a pair is dealt to 2, 4 or 8 workgroups.  A launch-shape choice: the arithmetic does not depend on it.
int wm_dec_attn_splits(int B, int H, const WmTuning &t);
// Split of K over the waves of a workgroup: a function of K ONLY (never of the batch), so that the order in which a
// row's sum is formed -- and therefore every logit bit -- does not depend on the decode group the row is in.
// Returns the wave count; *spw = k-steps (of 32) per wave, one of {2, 4, 5, 6, 8, 10, 12}.
int wm_dec_gemv_split(int K, int *spw);
// the fused query + cross-attention launch applies: 96 .. 256 pairs, alone on the device, a K split it is built for
bool wm_dec_xattn_fq_applies(int B, int H, int K, bool short_lived, const WmTuning &t);

// ---------------------------------------------------------------- attention plans ----
enum DecAttnVariant {
    DAV_STREAM = 0,       // dec_xrows_attn_kernel<8, 4, NT>, grid (workgroups, nsplit), 8 / nsplit waves
    DAV_FLAT = 1,         // dec_xrows_attn_kernel<8, 4, NT>, the flat deal (xattn_no_deep)
    DAV_FLAT_DEEP_C = 2,  // dec_rows_attn_kernel<8, 4, false, true>: flat deal, deep, cacheable loads
    DAV_FLAT_DEEP_NT = 3, // dec_rows_attn_kernel<8, 4, NT, true>: flat deal, deep, non-temporal loads
    DAV_SELF = 4,         // dec_rows_attn_kernel<4, 4, false>
    DAV_SELF_OFF = 5,     // dec_rows_attn_kernel<4, 4, false, false, true>: ragged rows
    DAV_SELF_PANEL = 6,   // dec_rows_attn_kernel<4, 4, false, false, false, true>
    DAV_CAND = 7,         // dec_xcand_attn_kernel<N, NT>, one 8-wave workgroup per pair, persistent
    DAV_CAND_FLAT = 8,    // dec_xcand_attn_kernel<N, NT>, the flat deal
    DAV_FQ = 9,           // dec_xattn_fq_kernel<spw, NT>
    DAV_SELF_OFF_PANEL = 10,   // dec_rows_attn_kernel<4, 4, false, false, true, true>: a prompt panel of ragged rows
};
// the integers of a DecAttnArgs (model.h); which fields a form reads is said at its plan function
struct DecAttnShape {
    int B;                 // rows (cross, self, fused-query)
    int C, N;              // windows x rows per window (candidate group, panel)
    int H, T_stride, n_keys;
    int nsplit;            // cross: workgroups per pair (1, 2, 4, 8)
    int K;                 // fused-query: K of the query projection
    bool has_pos, has_part, has_off, has_pf, short_lived;
    int pf_rows, pf_k;
};
struct DecAttnPlan {
    int variant;           // DecAttnVariant
    int spw;               // DAV_FQ: k-steps per wave of the query projection (its template argument), else 0
    int grid_x, grid_y, block;
    int lds;               // dynamic LDS bytes
    int n_wg;              // compute workgroups (grid_x without the warm-up tiles)
    int warm_tiles;        // L2 warm-up workgroups behind the compute ones
    long tile_bytes;       // bytes per warm-up tile
    DecAttnWords w;        // packA, packB, packC (c = 0 where the kernel takes none)
    int combine_grid;      // > 0: a dec_attn_combine_kernel<8> launch of this many workgroups follows
};
// Each returns WM_OK, or WM_ERR_INVALID with the message set (wm_set_error) for a geometry the launcher refuses.
// cross (wm_dec_attention): B, H, T_stride, n_keys, nsplit, has_part, short_lived, warm-up
int wm_plan_attention(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p);
// candidate group (wm_dec_attention_cand): C, N, H, T_stride, n_keys, has_part, short_lived, warm-up
int wm_plan_attention_cand(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p);
// fused query (wm_dec_xattn_fq): B, H, T_stride, n_keys, K, warm-up
int wm_plan_xattn_fq(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p);
// self (wm_dec_self_attention): B, H, T_stride, n_keys, has_pos, has_off, warm-up
int wm_plan_self_attention(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p);
// panel (wm_dec_self_attention_panel): C, N (= the width w), H, T_stride, has_pos, has_off (the windows' offsets), warm-up
int wm_plan_self_attention_panel(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p);

// ---------------------------------------------------------------- GEMV plan ----
struct DecGemvShape {
    int epi;               // DecEpi
    bool ln;               // LayerNorm mode
    int B, N, K;
    bool has_pf;
    int pf_rows, pf_k, pf_head_major;
};
struct DecGemvPlan {
    int nw, spw;           // waves over K and k-steps per wave (wm_dec_gemv_split)
    int tn, nblk;          // tiles and batch blocks per workgroup
    int ppw;               // K parts per wave: 2 = the two-part kernel on nw / 2 waves
    int row_split;         // 1: the residual epilogue is finished by four waves per unit
    int bgroups, n_tiles, n_tg, n_tg_pad;
    int grid, block;
    long lds;              // dynamic LDS bytes
    int pf_tiles;          // 0: no warm-up (the launcher passes no pointer then)
    long pf_tile_bytes;
    int pf_head_major;
};
int wm_plan_gemv(const DecGemvShape &s, int n_cus, const WmTuning &t, DecGemvPlan *p);

// flat int32 forms of the plans for the debug hooks (debug_hooks.cpp) and stand-alone checks: `in` / `out` layouts are
// documented at wmdbg_dec_attn_plan / wmdbg_dec_gemv_plan (include/whisper_mi355x_debug.h)
constexpr int WM_ATTN_PLAN_IN = 16, WM_ATTN_PLAN_OUT = 16, WM_GEMV_PLAN_IN = 12, WM_GEMV_PLAN_OUT = 20;
void wm_attn_plan_flat(const int32_t *in, const WmTuning &t, int32_t *out);
void wm_gemv_plan_flat(const int32_t *in, const WmTuning &t, int32_t *out);
