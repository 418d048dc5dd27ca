// tx_pending.h -- the state a setter arms "for the NEXT transcribe call, consumed by it whatever happens", as ONE value: the
// setters write WmModel::pending; a transcribe call begins by TAKING it -- before any check, so a call that fails has consumed
// it too -- and works on its own copy.  The debug library's one-shots ride in it.  Who serves which item is one pure function.
// Plain C++, no HIP, no context: tests/test_pending_cpu.py pins both on the CPU.  DESIGN.md section 4e.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "whisper_mi355x.h"

// The debug library's one-shots (null / -1 in the product): host memory that lives until the call returns.
struct WmDebugShots {
    float *align_matrix = nullptr;          // wmdbg_align_capture: the cost matrices [B][max_new + 1][1500] of an aligned call
    int align_hyp = -1;                     // wmdbg_align_hyp: an aligned best-of / beam call aligns hypothesis min(align_hyp, n_hyp - 1)
    int32_t *align_slots = nullptr;         // wmdbg_hyp_slots: where that call leaves its slot tables [B][Tq]
    float *beam_trace = nullptr;            // wmdbg_beam_trace: [B][max_new][n_cand][WM_BEAM_TRACE] of a beam call
    const int32_t *spec_script = nullptr;   // wmdbg_spec_script: a speculative call's proposals [spec_script_rows][spec_script_new]
    int spec_script_new = 0, spec_script_rows = 0;
};
enum : unsigned { WM_PEND_BUDGETS = 1, WM_PEND_BIAS_ROWS = 2, WM_PEND_CST_ROWS = 4, WM_PEND_SAMP_ROWS = 8, WM_PEND_ALT = 16, WM_PEND_GIVEN = 32 };
struct WmPending {   // (an empty list: none pending)
    std::vector<int32_t> budgets;               // wm_set_token_budgets: per chunk
    std::vector<int32_t> bias_rows, cst_rows;   // wm_set_bias_rows, wm_set_constraint_rows: the table / the start state of each row
    std::vector<float> samp_T;                  // wm_set_sampling_rows: temperature and seed of each row (one length)
    std::vector<uint64_t> samp_seed;
    bool alt_on = false;                        // wm_request_alternatives: a request is pending, and the request
    wm_alternatives_out alt = {};
    // wm_set_given_tokens: lens [n] and the tokens [n][given_stride] of the call's hypothesis rows (given_lens empty: none)
    std::vector<int32_t> given_lens, given_tok;
    int given_stride = 0;
    WmDebugShots dbg;
    WmPending take() { return std::exchange(*this, WmPending()); }   // the whole value; what stays behind is empty
    unsigned bits() const {
        return (budgets.empty() ? 0u : WM_PEND_BUDGETS) | (bias_rows.empty() ? 0u : WM_PEND_BIAS_ROWS) |
               (cst_rows.empty() ? 0u : WM_PEND_CST_ROWS) | (samp_T.empty() ? 0u : WM_PEND_SAMP_ROWS) | (alt_on ? WM_PEND_ALT : 0u) |
               (given_lens.empty() ? 0u : WM_PEND_GIVEN);
    }
};
inline const WmPending &wm_nothing_pending() { static const WmPending none; return none; }
// ---------------------------------------------------------------- who serves what ----
struct WmCallKind {   // what a call is, as far as the pending items care (a transcribe call's TxCall begins with it)
    enum Entry { PLAIN, MEL, RAGGED, BEST_OF, BEAM } entry = PLAIN;   // whose own checks run first
    bool greedy_entry = false;   // wm_transcribe_greedy: no options, so no per-row ones either (wm_set_sampling_rows is refused)
    int n_cand = 1;              // candidates per row (wm_transcribe_mel_best_of): every row decodes n_cand times over ONE encoder pass
    bool beam = false;           // wm_transcribe_mel_beam: the n_cand rows of a window are its BEAMS (n_cand = beam width, 1 included)
    bool windows = false;        // the rows are windows of an encoded set
    bool hyp = false;            // an aligned best-of / beam call: a window decodes n_cand rows and aligns hypothesis best_out[b] alone
    bool speculative = false, multi = false, f32_path = false;   // wm_transcribe_mel_speculative; wm_multi_transcribe_greedy; the all-f32 debug path
};
// Null when call k serves the items `pending` names (WM_PEND_* bits), else the message of its WM_ERR_STATE; alternatives are
// judged first, given tokens second.  Which error wins is part of the ABI, so a caller passes the items it answers for at that point: a transcribe
// call its sampling row map in front of the entry's own checks and its alternatives inside validation, the speculative and the
// multi entry both at once.  Every call serves budgets, and the other two row maps where it runs with what they map in force.
inline const char *wm_pending_refusal(unsigned pending, const WmCallKind &k) {
    if (pending & WM_PEND_ALT) {
        if (k.multi) return "multi_transcribe_greedy does not serve alternatives (wm_request_alternatives)";
        if (k.speculative) return "alternatives are not served by speculative decoding";
        if (k.beam) return "alternatives are not served by beam-search calls";
        if (k.f32_path) return "alternatives are not supported by the all-f32 precision path";
    }
    if (pending & WM_PEND_GIVEN) {   // served by the plain, mel, ragged, best-of and window-set entries and their aligned counterparts
        if (k.multi) return "multi_transcribe_greedy takes no given tokens (wm_set_given_tokens)";
        if (k.speculative) return "speculative decoding takes no given tokens (wm_set_given_tokens)";
        if (k.beam || k.entry == WmCallKind::BEAM) return "beam-search calls take no given tokens (wm_set_given_tokens)";
        if (k.greedy_entry) return "wm_transcribe_greedy takes no given tokens (wm_set_given_tokens): it has no log-prob output";
        if (k.hyp) return "aligned best-of calls take no given tokens (wm_set_given_tokens)";
        if (k.f32_path) return "given tokens are not supported by the all-f32 precision path";
    }
    if (pending & WM_PEND_SAMP_ROWS) {   // served by the plain, mel, ragged, window-set and aligned entries
        if (k.multi) return "multi_transcribe_greedy takes no sampling row map (wm_set_sampling_rows)";
        if (k.speculative) return "speculative decoding takes no sampling row map (wm_set_sampling_rows)";
        if (k.greedy_entry) return "wm_transcribe_greedy takes no sampling row map (wm_set_sampling_rows)";
        // (wm_transcribe_windows is the best-of entry of a window set: one sample per row is the plain call)
        const bool one_sample = k.entry == WmCallKind::BEST_OF && k.windows && k.n_cand == 1 && !k.hyp;
        if ((k.entry == WmCallKind::BEST_OF || k.entry == WmCallKind::BEAM) && !one_sample)
            return "best-of and beam-search calls take no sampling row map (wm_set_sampling_rows)";
        if (k.f32_path) return "a sampling row map is not supported by the all-f32 precision path";
    }
    return nullptr;
}
