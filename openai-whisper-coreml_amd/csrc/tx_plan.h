// tx_plan.h -- the host arithmetic of a transcribe call as pure functions (tx_plan.cpp).
//
// What transcribe.cpp decides before it touches the device, and what it computes from a group's fetched streams after: how a
// call of B rows is cut into decode groups and which lanes run them (wm_tx_plan and its four ingredients), the tables a group
// uploads (wm_group_tables) and the rows of the call's outputs a finished group fills (wm_group_rows_out).  Plain C++, no HIP
// headers, no context, no global state -- the tuning knobs are passed in -- so tests/test_tx_plan_cpu.py pins every rule on the
// CPU (wmdbg_tx_plan / wmdbg_group_tables / wmdbg_group_rows_out) against the restatement in tests/tx_plan_ref.py.
#pragma once
#include <stdint.h>

#include <vector>

#include "dec_launch.h"   // WM_DEC_MAXB
#include "wm_tuning.h"

// ---------------------------------------------------------------- decode groups and lanes ----
// Decode groups of a call of B chunks on at most L lanes.  explicit_lanes: the host set a lane count (wm_set_lanes n > 0);
// gc_probe: the debug knob group_chunks (0 in the product).
int wm_group_count(int B, int L, bool explicit_lanes, int gc_probe);
// B rows in G balanced runs: run g is rows [b0[g], b0[g] + cg[g])
void wm_balanced_cut(int B, int G, std::vector<int> &b0, std::vector<int> &cg);
// ... of a candidate call (wm_transcribe_mel_best_of) of B windows x N candidates: groups of whole windows; returns their number
int wm_cand_groups(int B, int N, int L, bool explicit_lanes, std::vector<int> &b0, std::vector<int> &cg);
// CU-masked groups of a call (0: none -- unmasked lanes as wm_group_count says; 2 / 3: that many groups, one per part of the chip)
int wm_lane_parts(int B, int L, bool explicit_lanes, int n_text_state, int n_text_layer, const WmTuning &t);

// the contexts a call's lanes run on: the caller's context and its clones, the CU-masked clones of a partition of the chip,
// or (probes) one clone confined to a few CUs
enum WmLaneKind { WM_LANES_CLONES = 0, WM_LANES_PARTS = 1, WM_LANES_SOLO = 2 };

struct WmTxPlanIn {
    int B = 1;                    // rows of the call (a candidate call: windows)
    int N = 1;                    // candidates (beams) per row
    int lanes = 1;                // the lane limit: wm_set_lanes' count when the host set one, else the default
    bool explicit_lanes = false;  // the host set it
    bool prof_on = false;         // per-kernel profiling: everything on the caller's context
    bool no_cu_masks = false;     // this device refused a CU-masked stream before
    int n_text_state = 0;
    // Upper bound on the rows (candidate call: windows x N decoder rows) of ONE group; 0: none.  An aligned call's capture
    // budget (wm_transcribe_mel_aligned): at least ceil(B / bound) balanced groups, and no sub-chip parts when they would be
    // too few.  With 0 the plan is what it was before the bound existed.
    int max_group_rows = 0;
};

struct WmTxPlan {
    int L = 1;              // lanes the call may use
    int parts = 0;          // 2 / 3: sub-chip lanes
    int G = 1;              // decode groups: group g is rows (windows) [b0[g], b0[g] + cg[g])
    std::vector<int> b0, cg;
    int n_lanes = 1;        // lanes that run: more groups than lanes go in rounds
    WmLaneKind kind = WM_LANES_CLONES;
};

// The composite decision, once.  Reads lane_parts, lane_solo_cus and group_chunks of the tuning.
void wm_tx_plan(const WmTxPlanIn &in, const WmTuning &t, WmTxPlan *out);

// ---------------------------------------------------------------- a group's tables ----
// the prompts of a call: row b's is prompt + b * stride (stride 0: one prompt for all)
struct TxPrompts {
    const int32_t *prompt = nullptr;
    int stride = 0;
    const int32_t *len = nullptr;   // non-null: a ragged call, row b's prompt is its first len[b] entries
    int sot_tail = 0;               // ... whose <|startoftranscript|> is entry len[b] - sot_tail
    const uint32_t *sample_ids = nullptr;
};

// what a group uploads before its first position (sources of asynchronous copies: they live in the lane's job)
struct TxGroupTables {
    std::vector<int32_t> pr;     // prompt tokens [P][Bg], position-major like dseq
    std::vector<int32_t> off;    // a ragged call: row offsets [Bg] = P - len
    std::vector<int32_t> bud;    // token budgets [Bg] (a call with budgets)
    std::vector<unsigned> ids;   // a candidate group: [2][ids_stride] window ids | candidate words; else the rows' sample ids [Bg]
    std::vector<int32_t> glen, gtok;   // given tokens (wm_set_given_tokens): lens [Bg], tokens [Bg][L] (wm_group_given)
    std::vector<int32_t> sbr;    // row tables (wm_set_bias_rows): [Bg][2] (first group, end group) of each row's table in the pool
};

// the right-aligned prompt table [P][Bg] and the row offsets [Bg] of rows [b0, b0 + Bg) of a ragged call; returns P
int wm_right_align(const int32_t *prompts, int stride, const int32_t *prompt_len, int b0, int Bg, std::vector<int32_t> &table,
                   std::vector<int32_t> &off);
// The tables of the group of rows (windows) [b0, b0 + Cg) x N candidates: decoder row b belongs to window b / N and is its
// candidate b % N.  n_prompt: the prompt length of a uniform call; budgets: [B] of the call (null: none); want_ids: the
// extended decode is on.  Returns P, the group's prompt positions (a ragged call: the longest prompt among ITS rows).
int wm_group_tables(const TxPrompts &p, int n_prompt, const int32_t *budgets, int b0, int Cg, int N, int ids_stride, bool want_ids,
                    TxGroupTables *out);

// The per-row group ranges of the same group under row tables (wm_set_sequence_bias_tables): decoder row b takes the table of
// window b0 + b / N of the call -- table_of_row [B] of the call, -1: none; tab_grp [n_tables + 1]: table t is groups
// [tab_grp[t], tab_grp[t + 1]) of the pool.  out [Bg][2]; a row without a table gets (0, 0).  An index outside [-1, n_tables)
// is the caller's to refuse; here it reads as none.
void wm_group_bias_rows(const int32_t *table_of_row, const int32_t *tab_grp, int n_tables, int b0, int Cg, int N,
                        std::vector<int32_t> *out);

// The given tokens of the same group (wm_set_given_tokens): decoder row b is hypothesis row b0 * N + b of the call -- lens [B * N],
// tok [B * N][stride] of the call.  lens_out [Bg], tok_out [Bg][L] with L = the group's longest given text (at least 1; the
// tail of a shorter row repeats its last given token, a free row reads 0).  Returns L, or 0 when no row of the group is given:
// such a group makes the launches of a call without a table.
int wm_group_given(const int32_t *lens, const int32_t *tok, int stride, int b0, int Cg, int N, std::vector<int32_t> *lens_out,
                   std::vector<int32_t> *tok_out);

// ---------------------------------------------------------------- a group's outputs ----
// The output rows of a finished plain (not beam) group from its fetched streams gen [max_new][Bg], lp [max_new][Bg] (read
// when logprobs is given) and ns [Bg] (when no_speech is): decoder row b is output row b0 * N + b.  A row ends at its budget
// or with its first eot; tokens past the end read eot, log-probs 0 -- the stopping token has its log-prob, nothing after it.
void wm_group_rows_out(const int32_t *gen, const float *lp, const float *ns, const int32_t *budgets, int32_t eot, int N, int b0,
                       int Bg, int max_new, int32_t *tokens, int32_t *lens, float *logprobs, float *no_speech);
// The same rows' alternatives (wm_request_alternatives) from the fetched tok / lp [max_new][Bg][n] and cnt / ent [max_new][Bg],
// by the same row map, into tokens / logprobs [rows][max_new][n] and counts / entropy [rows][max_new] (both nullable).  lens:
// the call's, as wm_group_rows_out wrote them -- every position at or past a row's length is a pad (id -1, log-prob 0, count 0,
// entropy 0), whatever the device left there.
void wm_group_alt_out(const int32_t *tok, const float *lp, const int32_t *cnt, const float *ent, int n, int N, int b0, int Bg,
                      int max_new, const int32_t *lens, int32_t *tokens, float *logprobs, int32_t *counts, float *entropy);

// ---------------------------------------------------------------- speculative decoding ----
// wm_transcribe_mel_speculative.  The decode groups of a call of B windows at draft length k: a verify
// step holds G x (k + 1) <= WM_DEC_MAXB rows, and below that bound the lockstep cut trades group size against acceptance --
// spec_group (WmTuning; 0: the measured default) is the preferred group size.  Balanced runs; returns their number.
int wm_spec_groups(int B, int k, int spec_group, std::vector<int> &b0, std::vector<int> &cg);
// The width of the next verify step: draft length k, `bound` = an upper bound on the group's device position, `last` = the last
// position a row may have (n_prompt + max_new - 2).  0: no row is left, or the bound is too loose to tell -- ask the device.
int wm_spec_width(int k, int bound, int last);
// One round of a group of G windows whose verify step had w rows per window: accepted[c] leading rows matched, live[c] != 0 =
// the window was live, eot_at[c] / left[c]: spec_round.h.  Returns n, the positions the group advances (0: nobody is live);
// live_out[c], and inc [G][4] = the increments of wm_spec_stats (rounds, proposed, accepted, kept; zero for a frozen window).
int wm_spec_round(int G, int w, const int32_t *accepted, const int32_t *live, const int32_t *eot_at, const int32_t *left,
                  int32_t *live_out, int32_t *inc);

// ---------------------------------------------------------------- prompt panels ----
// wm_set_prompt_panel: the prompt positions of a plain decode group whose logits nobody reads run as
// teacher-forced panel steps -- `width` positions of the same sequences per decoder step, no logits product, no close.
constexpr int WM_PANEL_MAX_WIDTH = 8;   // = WM_MAX_TEACHER_PANEL (model.h asserts it)
// How a group of G windows is cut for a panel pass of T positions at `width`: *C windows per slice, *w <= width positions per
// panel, C * w <= WM_DEC_MAXB -- the cut with the fewest steps (the rule and its measurements: model.cpp
// wm_model_panel_slices, which passes the probe knob teacher_panel_cut; 0 = the rule).
void wm_panel_slices(int G, int width, int T, int knob, int *C, int *w);
struct WmPromptPanelPlan {
    int P0 = 0;       // the first position whose logits the call reads: the group's first ordinary step
    int C = 0, w = 0; // windows per slice, positions per panel (0: no prefill -- every position is an ordinary step)
    int slices = 0;   // slices of the group
    int steps = 0;    // panel steps per slice: ceil(P0 / w), the last one narrower when w does not divide P0
};
// The rule.  P: the group's prompt positions (a ragged group: its longest prompt); sot_pos: the <|startoftranscript|> position
// when the call computes no_speech_prob, else -1; acap_base: an aligned group's first captured position, else -1.
// P0 = sot_pos when given, else P - 1; an aligned group caps it at acap_base.  Positions [0, P0) only fill the self-attention
// cache.  width <= 1 or P0 < 2: no prefill (C = w = slices = steps = 0) -- the lane enqueues exactly what it always did.
void wm_prompt_panel_plan(int G, int width, int P, int sot_pos, int acap_base, int knob, WmPromptPanelPlan *out);

// ---------------------------------------------------------------- given panels ----
// wm_set_given_panel: the positions of a plain decode group at which every row either decodes a given
// token (wm_set_given_tokens) or is finished for a reason the host knows run as panel rounds of up to `width` positions per
// decoder step, closed by given_panel.hip.  Why a group is not served, in the order the rule tests (the first that applies):
enum WmGivenPanelReason {
    WM_GP_SERVED = 0,
    WM_GP_WIDTH1,      // the setting is at its default
    WM_GP_NO_TABLE,    // no row of the group is given
    WM_GP_CANDIDATES,  // a best-of or beam group
    WM_GP_RAGGED,      // ragged prompts
    WM_GP_NO_X,        // the extended decode is off
    WM_GP_SAMP_ROWS,   // a sampling row map
    WM_GP_TRUNC,       // temperature > 0 under the sampling rules
    WM_GP_ALT,         // alternatives
    WM_GP_SB_TABLES,   // sequence-bias row tables
    WM_GP_SB,          // a sequence bias
    WM_GP_CST,         // a constraint
    WM_GP_REP,         // repetition rules
    WM_GP_ACAP,        // an aligned group
    WM_GP_F32,         // the all-f32 path, or debug hooks staged by the caller
    WM_GP_NARROW,      // min(width, 128 / G) < 2
    WM_GP_NO_PHASE,    // Lp <= 1: generated index 1 is neither given nor finished for some row
    WM_GP_REASONS
};
// the mode of the group as the rule reads it (one bit each; wmdbg_given_panel_plan takes the same word)
enum WmGivenPanelBits {
    WM_GPB_GIVEN = 1 << 0, WM_GPB_CAND = 1 << 1, WM_GPB_OFF = 1 << 2, WM_GPB_X = 1 << 3, WM_GPB_SROWS = 1 << 4, WM_GPB_TRUNC = 1 << 5,
    WM_GPB_ALT = 1 << 6, WM_GPB_SBT = 1 << 7, WM_GPB_SB = 1 << 8, WM_GPB_CST = 1 << 9, WM_GPB_REP = 1 << 10, WM_GPB_ACAP = 1 << 11,
    WM_GPB_F32 = 1 << 12, WM_GPB_SAMPLE = 1 << 13
};
struct WmGivenPanelPlan {
    int reason = WM_GP_WIDTH1;   // WM_GP_SERVED: the phase runs
    int w = 0;                   // rows per window of a full round: min(width, 128 / G) (0: not served before the width was looked at)
    int Lp = 0;                  // generated indices [1, Lp) are the phase (0 / 1: none)
    int rounds = 0;              // ceil((Lp - 1) / w), the last one min(w, Lp - g0) wide
};
// The rule (include/whisper_mi355x.h states it in full).  G rows; lens [G]: the rows' given tokens; budgets [G] or null: the
// rows' token budgets; P: the group's prompt positions; bits: WmGivenPanelBits (WM_GPB_SAMPLE: the call samples, temperature > 0).
// Lp = the largest L <= max_new with P + L - 1 < n_text_ctx such that for every row r and every gi in [1, L): gi < lens[r] or
// gi >= min(budget[r], max_new).
void wm_given_panel_plan(int G, int width, const int32_t *lens, const int32_t *budgets, int max_new, int P, int n_text_ctx, unsigned bits,
                         WmGivenPanelPlan *out);

// ---------------------------------------------------------------- the hooks' flat forms ----
// documented at wmdbg_tx_plan / wmdbg_group_tables / wmdbg_group_rows_out (include/whisper_mi355x_debug.h)
constexpr int WM_TX_PLAN_IN = 12, WM_TX_PLAN_OUT = 8;
constexpr int WM_TX_TAB_IN = 256, WM_TX_TAB_OUT = 576, WM_TX_TAB_ROWS = 16, WM_TX_TAB_POS = 12;
constexpr int WM_TX_ROWS_IN = 320, WM_TX_ROWS_OUT = 288, WM_TX_ROWS_NEW = 8;
// returns the entries written to cut (b0[0 .. G), cg[0 .. G)), or -1 when they do not fit cut_cap
// (max_group_rows: WmTxPlanIn's, not part of the flat input -- wmdbg_tx_plan_bounded passes it beside)
int wm_tx_plan_flat(const int32_t *in, int32_t *out, int32_t *cut, int cut_cap, int max_group_rows = 0);
bool wm_group_tables_flat(const int32_t *in, int ids_stride, int32_t *out);
bool wm_group_rows_out_flat(const int32_t *in, int32_t *out);
