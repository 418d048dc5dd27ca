"""Given tokens (wm_set_given_tokens) restated in f64 numpy on alt_ref.py's admissible set and sum rule --
tests/test_given_cpu.py, tests/test_given_kernel_gpu.py and tests/test_given_gpu.py read this one file.

One row's given step: the close takes the given id whatever the row would have chosen.  Its log-prob is v(id) - logsumexp(A)
with A the admissible set of the decision the row would have made WITHOUT the table (when the sum rule forces a timestamp, the
admissible timestamps alone), and -inf where the id is not in A: outside the row's ranges, a text id under a forced timestamp,
suppressed or banned (a ban is a suppressed id here), v = -inf or NaN.  A row with nothing admissible is not touched."""
import types

import numpy as np

import alt_ref as A

# (V, B) of the kernel test: the ragged last tile, the row-count boundaries 16 / 17 / 128 of the close, the real vocabulary
SHAPES = [(1030, 1), (1030, 6), (1024, 17), (1024, 128), (51865, 16)]
CASES = ("admissible text, not forced", "admissible text, forced", "admissible timestamp, not forced",
         "admissible timestamp, forced", "inadmissible text, not forced", "inadmissible text, forced",
         "inadmissible timestamp, not forced", "inadmissible timestamp, forced", "timestamp rules off")


def given_np(v, tok, suppress=(), rng=None, ts_begin=None):
    """One row: namespace(logprob f64 or -inf, forced, admissible, touched, case).  touched False: nothing is admissible, the
    library leaves the row to the close's own path.  case: one of CASES ("text" means: not a timestamp of a call with rules; a
    text id that the sum rule alone excludes counts as inadmissible, as the header says)."""
    v64 = np.asarray(v, np.float64)
    ok, gap = A.admissible(v64, suppress, rng)
    forced = gap is not None and gap > 0
    if not ok.any():
        return types.SimpleNamespace(logprob=-np.inf, forced=forced, admissible=False, touched=False, case=None)
    adm = bool(ok[tok])
    lp = -np.inf
    if adm:
        m = v64[ok].max()
        lp = float(v64[tok] - (m + np.log(np.exp(v64[ok] - m).sum())))
    if rng is None:
        case = CASES[8]
    else:   # (the case names judge the id before the sum rule: "admissible text, forced" is a text id the rule alone excludes)
        base = v64[tok] > -np.inf and tok not in set(int(s) for s in suppress) and \
            (rng[0] <= tok < rng[1] or rng[2] <= tok < rng[3])
        kind = "timestamp" if tok >= ts_begin else "text"
        case = "%s %s, %s" % ("admissible" if base else "inadmissible", kind, "forced" if forced else "not forced")
    return types.SimpleNamespace(logprob=lp, forced=forced, admissible=adm, touched=True, case=case)


def ts_advance_np(hist, tok, ts_begin, eot, V):
    """dec_close.h's ts_advance: (the history after `tok`, the ranges (text_lo, text_hi, ts_lo, ts_hi) of the next position)"""
    n, last_is, prev_is, last_val = (int(x) for x in hist)
    prev_ts = n < 1 or last_is != 0
    last_ts = tok >= ts_begin
    val = int(tok) if last_ts else last_val
    text_lo, text_hi, ts_lo, ts_hi = 0, ts_begin, ts_begin, V
    if last_ts:
        if prev_ts:
            ts_hi = ts_lo
        else:
            text_lo = eot
    if val >= 0:
        ts_lo = max(ts_lo, val if (last_ts and not prev_ts) else val + 1)
    return [n + 1, int(last_ts), last_is, val], [text_lo, text_hi, ts_lo, ts_hi]


def group_given_np(lens, tok, b0, Cg, N):
    """tx_plan.cpp's wm_group_given: (L, lens [Bg], tok [Bg][max(L, 1)]) of the group of windows [b0, b0 + Cg) x N"""
    lens, tok = np.asarray(lens, np.int32), np.asarray(tok, np.int32)
    r0, Bg = b0 * N, Cg * N
    gl = lens[r0:r0 + Bg].copy()
    L = int(gl.max())
    gt = np.zeros((Bg, max(L, 1)), np.int32)
    for b in range(Bg):
        n = int(gl[b])
        if n > 0:
            gt[b, :n] = tok[r0 + b, :n]
            gt[b, n:] = tok[r0 + b, n - 1]
    return L, gl, gt
