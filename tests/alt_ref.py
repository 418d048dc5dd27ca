"""Top-n alternatives and entropy (wm_request_alternatives) restated in f64 numpy, and the seeded rows
the kernel tests run on -- tests/test_alternatives_cpu.py and tests/test_alternatives_kernel_gpu.py read this one list.

The rules, per row: the admissible set A is what the suppress list and the timestamp ranges (text_lo, text_hi, ts_lo, ts_hi)
leave; when the summed probability of the admissible timestamps exceeds the best admissible text token (the sum rule), A is
the admissible timestamps alone; ids whose value is -inf (or NaN) are not in A.  The list is A by descending value, equal
values lower id first; log-probs are v - logsumexp(A); the count is min(n, |A|); the entropy is -sum p log p over A."""
import types

import numpy as np

MAX_ALTERNATIVES = 16
PAD_ID = -1

# (V, n, rows) of the kernel test: an odd vocabulary, the real ones, more rows than one wave's ballot, no multiple of the tile
SHAPES = [(1024, 5, 10), (51865, 16, 16), (51864, 1, 7), (1030, 3, 6), (1024, 8, 128), (51865, 4, 17)]
# the smallest |lse(timestamps) - best text| a seeded row may have: below it f32 and f64 may decide the sum rule differently
MIN_SUM_RULE_GAP = 0.04


def admissible(v, suppress, rng):
    """(mask of A, sum-rule gap lse(ts) - best text; +-inf where one side is empty, None without timestamp rules)"""
    v = np.asarray(v, np.float64)
    ok = np.ones(v.size, bool)
    if len(suppress):
        ok[np.asarray(suppress, np.int64)] = False
    gap = None
    if rng is not None:
        tl, th, sl, sh = (int(x) for x in rng)
        text = np.zeros(v.size, bool)
        text[tl:th] = True
        ts = np.zeros(v.size, bool)
        ts[sl:sh] = True
        text &= ok
        ts &= ok
        gap = -np.inf
        if ts.any():
            m = v[ts].max()
            lse_ts = m + np.log(np.exp(v[ts] - m).sum()) if np.isfinite(m) else -np.inf
            best_text = v[text].max() if text.any() else -np.inf
            gap = np.inf if not text.any() else lse_ts - best_text
            if gap > 0:
                text[:] = False
        ok = text | ts
    with np.errstate(invalid="ignore"):
        ok &= v > -np.inf
    return ok, gap


def alternatives_np(v, n, suppress=(), rng=None):
    """One row: namespace(ids [count], logprobs [count] f64, count, entropy f64, gap, size = |A|)."""
    v64 = np.asarray(v, np.float64)
    ok, gap = admissible(v64, suppress, rng)
    ids = np.flatnonzero(ok)
    if ids.size == 0:
        return types.SimpleNamespace(ids=np.zeros(0, np.int64), logprobs=np.zeros(0), count=0, entropy=0.0, gap=gap, size=0)
    m = v64[ids].max()
    lse = m + np.log(np.exp(v64[ids] - m).sum())
    lp = v64[ids] - lse
    order = np.lexsort((ids, -v64[ids]))
    top = order[:n]
    return types.SimpleNamespace(ids=ids[top], logprobs=lp[top], count=int(top.size), entropy=float(-(np.exp(lp) * lp).sum()),
                                 gap=gap, size=int(ids.size))


def packed(rows_ref, n):
    """The references of some rows as the library packs them: tokens [rows][n] (-1 pads), logprobs (0 pads), counts, entropy."""
    R = len(rows_ref)
    tok = np.full((R, n), PAD_ID, np.int32)
    lp = np.zeros((R, n), np.float64)
    cnt = np.zeros(R, np.int32)
    ent = np.zeros(R, np.float64)
    for b, r in enumerate(rows_ref):
        tok[b, :r.count] = r.ids
        lp[b, :r.count] = r.logprobs
        cnt[b] = r.count
        ent[b] = r.entropy
    return tok, lp, cnt, ent


def seeded_rows(V, rows):
    """The rows of one shape, by the recipe of tests/test_beam_kernel_gpu.py: N(0, 3^2) logits, 60 suppressed ids, 20 -inf in row
    0, a three-way tie at the top of row 1, suppressed ids at 50.0 in row 2; with the timestamp rules on, ranges by b % 5 and the
    timestamps of rows 3::5 boosted by 6.  namespace(logits, logits_ts, suppress, rng, ts_begin)."""
    g = np.random.default_rng(1000003 * V + rows)
    logits = (g.standard_normal((rows, V)) * 3.0).astype(np.float32)
    ts_begin = V - 124
    suppress = np.unique(g.integers(0, V, size=60)).astype(np.int32)
    logits[0, g.integers(0, V, size=20)] = -np.inf
    if rows > 1:
        top3 = np.argsort(-logits[1])[:3]
        logits[1, top3] = logits[1, top3[0]]
    if rows > 2:
        logits[2, suppress[:5]] = 50.0
    r4 = np.zeros((rows, 4), np.int32)
    for b in range(rows):
        kind = b % 5
        lo = ts_begin + int(g.integers(0, 60))
        if kind == 0:
            r4[b] = (0, 0, ts_begin, ts_begin + 21)
        elif kind == 1:
            r4[b] = (0, ts_begin, lo, lo)
        elif kind == 2:
            r4[b] = (ts_begin - 10, ts_begin, lo, V)
        else:
            r4[b] = (0, ts_begin, lo, V)
    boost = logits.copy()
    boost[3::5, ts_begin:] += np.float32(6.0)
    return types.SimpleNamespace(V=V, rows=rows, logits=logits, logits_ts=boost, suppress=suppress, rng=r4, ts_begin=ts_begin)


def case_inputs(s, ts_on):
    """(logits, rng or None) of one seeded shape with the timestamp rules off / on"""
    return (s.logits_ts, s.rng) if ts_on else (s.logits, None)


def case_reference(s, n, ts_on, rows=None):
    lg, rng = case_inputs(s, ts_on)
    idx = range(s.rows) if rows is None else rows
    return [alternatives_np(lg[b], n, s.suppress, None if rng is None else rng[b]) for b in idx]


def min_sum_rule_gap(s):
    """the smallest finite |gap| among the rows of a seeded shape under the timestamp rules"""
    gaps = [abs(alternatives_np(s.logits_ts[b], 1, s.suppress, s.rng[b]).gap) for b in range(s.rows)]
    gaps = [x for x in gaps if np.isfinite(x)]
    return min(gaps) if gaps else np.inf
