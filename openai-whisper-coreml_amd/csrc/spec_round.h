// spec_round.h -- the arithmetic of one round of a speculative decode group (wm_transcribe_mel_speculative, DESIGN.md section
// 18), stated ONCE for the device (spec.hip spec_commit_kernel) and the host (tx_plan.cpp wm_spec_round, which the tests pin
// against tests/spec_ref.py).  Plain C++: no HIP headers.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WM_SPEC_HD __host__ __device__
#else
#define WM_SPEC_HD
#endif

constexpr int WM_SPEC_NO_CUT = 1 << 30;

// A verify step of w rows per window closed with `accepted` leading rows whose winner equals the proposal: the window has
// accepted + 1 correct tokens (row `accepted`'s winner is the target's own next token).  eot_at = the index among them of the
// first end-of-text token (-1: none, or early stop on eot is off), left >= 1 = the tokens its budget still allows.
// The tokens the window would write if nothing but itself cut it short:
WM_SPEC_HD inline int wm_spec_window_own(int accepted, int eot_at, int left) {
    int m = accepted + 1;
    if (eot_at >= 0 && eot_at + 1 < m) m = eot_at + 1;
    if (left < m) m = left;
    return m < 0 ? 0 : m;
}
// ... and whether it is finished after them
WM_SPEC_HD inline int wm_spec_window_stops(int m, int eot_at, int left) { return ((eot_at >= 0 && eot_at < m) || left <= m) ? 1 : 0; }
// What the window asks of the group's lockstep cut n = min over the live windows: its correct tokens -- or nothing, when it
// finishes among them anyway (a window that stops leaves the min: whatever n is, it is done or still correct after n tokens).
WM_SPEC_HD inline int wm_spec_window_ask(int accepted, int eot_at, int left) {
    const int m = wm_spec_window_own(accepted, eot_at, left);
    return wm_spec_window_stops(m, eot_at, left) ? WM_SPEC_NO_CUT : accepted + 1;
}
// What a LIVE window makes of the cut n: *m = the tokens it writes (the stopping token included), *stop = it is finished after
// them; the statistics' *acc = the proposals among its own tokens, *kept = those among the tokens it writes.
WM_SPEC_HD inline void wm_spec_window_cut(int n, int accepted, int eot_at, int left, int *m, int *stop, int *acc, int *kept) {
    const int own = wm_spec_window_own(accepted, eot_at, left);
    const int mm = n < own ? n : own;
    *m = mm;
    *stop = wm_spec_window_stops(mm, eot_at, left);
    *acc = accepted < own ? accepted : own;
    *kept = accepted < mm ? accepted : mm;
}
