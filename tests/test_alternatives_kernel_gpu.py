"""Kernel-level tests of the alternatives kernel (csrc/alternatives.hip; wm_request_alternatives) through
the debug hook wmdbg_alternatives -- the kernel alone on the seeded rows of tests/alt_ref.py -- against the f64 restatement
there, against wmdbg_beam_topk (which calls the same list scan, row_list.h) bit for bit, and against itself across n and
across the group's shape.

Tolerances: ids and counts are exact (the selection compares f32 bits; no row of the seeded draws has a sum-rule gap below
alt_ref.MIN_SUM_RULE_GAP, which the test asserts, so no row is skipped).  Log-probs: 2e-4 absolute against f64, the gate of
tests/test_beam_kernel_gpu.py for this quantity.  Entropy: 2e-4 * max(1, H) against f64 -- the error source is the same
normaliser.  Largest values measured on the GPU over the twelve cases of the first test (one MI355X): log-prob 7.9e-7,
entropy 7.6e-7 relative to max(1, H), H up to 7.19 nats -- what an f32 restatement on the CPU gives (6.2e-7), far below the
5e-5 above which the error would need an explanation."""
import ctypes

import numpy as np
import pytest

import alt_ref as A

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
SENT_I, SENT_F = -77, np.float32(-123.25)
LIST = 9   # WM_MAX_BEAM + 1


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_alternatives.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, ctypes.c_int32, vp, vp, vp, vp]
    c.lib.wmdbg_alternatives.restype = ip
    c.lib.wmdbg_beam_topk.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, ctypes.c_int32, vp, vp, vp]
    c.lib.wmdbg_beam_topk.restype = ip
    yield c
    c.close()


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


_seeded = {}


def seeded(V, rows):
    """(the rows of one shape, computed once and left unchanged)"""
    if (V, rows) not in _seeded:
        _seeded[(V, rows)] = A.seeded_rows(V, rows)
    return _seeded[(V, rows)]


def run(dbg, logits, n, suppress, rng, ts_begin, counts=True, entropy=True):
    """The hook on sentinel-filled outputs: (counts or None, tokens, logprobs, entropy or None)"""
    logits = np.ascontiguousarray(logits, np.float32)
    rows, V = logits.shape
    tok = np.full((rows, n), SENT_I, np.int32)
    lp = np.full((rows, n), SENT_F, np.float32)
    cnt = np.full(rows, SENT_I, np.int32) if counts else None
    ent = np.full(rows, SENT_F, np.float32) if entropy else None
    sup = np.ascontiguousarray(suppress, np.int32)
    r4 = None if rng is None else np.ascontiguousarray(rng, np.int32)
    st = dbg.lib.wmdbg_alternatives(dbg.handle, _p(logits), rows, V, n, _p(sup) if sup.size else None, sup.size, _p(r4), ts_begin,
                                    _p(cnt), _p(tok), _p(lp), _p(ent))
    assert st == 0, dbg.lib.wm_last_error()
    return cnt, tok, lp, ent


def run_case(dbg, s, n, ts_on, rows=None, **kw):
    lg, rng = A.case_inputs(s, ts_on)
    if rows is not None:
        lg, rng = lg[rows], None if rng is None else rng[rows]
    return run(dbg, lg, n, s.suppress, rng, s.ts_begin, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_pads(cnt, tok, lp):
    """entries at and past the count are pads, entries below it are not; no sentinel is left anywhere"""
    n = tok.shape[1]
    past = np.arange(n)[None, :] >= cnt[:, None]
    assert np.all(tok[past] == A.PAD_ID) and np.all(bits(lp[past]) == 0)
    assert np.all(tok[~past] >= 0) and not np.any(tok == SENT_I) and not np.any(lp == SENT_F) and not np.any(cnt == SENT_I)


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
@pytest.mark.parametrize("V,n,rows", A.SHAPES)
def test_lists_counts_logprobs_and_entropy_against_f64(dbg, V, n, rows, ts_on):
    s = seeded(V, rows)
    if ts_on:
        assert A.min_sum_rule_gap(s) >= A.MIN_SUM_RULE_GAP   # no row's sum rule is within rounding: none is skipped
    cnt, tok, lp, ent = run_case(dbg, s, n, ts_on)
    ref = A.case_reference(s, n, ts_on)
    want_tok, want_lp, want_cnt, want_ent = A.packed(ref, n)
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(tok, want_tok), np.argwhere(tok != want_tok)[:5]
    check_pads(cnt, tok, lp)
    lp_err = float(np.abs(lp.astype(np.float64) - want_lp).max())
    ent_err = float((np.abs(ent.astype(np.float64) - want_ent) / np.maximum(1.0, want_ent)).max())
    print("V %d n %d rows %d ts %d: max |dlogprob| %.3g, max |dH| / max(1, H) %.3g (H up to %.3f)" %
          (V, n, rows, ts_on, lp_err, ent_err, want_ent.max()))
    assert lp_err <= 2e-4
    assert ent_err <= 2e-4
    assert np.all(np.diff(lp, axis=1)[np.arange(n - 1)[None, :] < cnt[:, None] - 1] <= 0)
    if ts_on:
        assert sum(1 for r in ref if r.gap is not None and r.gap > 0) >= 2   # rows where the sum rule forced a timestamp


def beam_lists(dbg, s, N, ts_on):
    """wmdbg_beam_topk over all rows of a shape: the hook takes whole windows of N beams, so the rows go in as a run of whole
    windows from row 0 and, when that leaves a tail, the last N rows (rows are independent)."""
    lg, rng = A.case_inputs(s, ts_on)
    out_n = np.zeros(s.rows, np.int32)
    out_t = np.zeros((s.rows, LIST), np.int32)
    out_l = np.zeros((s.rows, LIST), np.float32)
    spans = [(0, s.rows - s.rows % N)] if s.rows >= N else []
    if s.rows % N:
        assert s.rows >= N
        spans.append((s.rows - N, s.rows))
    for lo, hi in spans:
        if hi <= lo:
            continue
        part = np.ascontiguousarray(lg[lo:hi])
        r4 = None if rng is None else np.ascontiguousarray(rng[lo:hi])
        ln = np.full(hi - lo, -1, np.int32)
        lt = np.full((hi - lo, LIST), -1, np.int32)
        ll = np.full((hi - lo, LIST), np.nan, np.float32)
        st = dbg.lib.wmdbg_beam_topk(dbg.handle, _p(part), hi - lo, s.V, N, _p(s.suppress), s.suppress.size, _p(r4), s.ts_begin,
                                     _p(ln), _p(lt), _p(ll))
        assert st == 0, dbg.lib.wm_last_error()
        out_n[lo:hi], out_t[lo:hi], out_l[lo:hi] = ln, lt, ll
    return out_n, out_t, out_l


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
@pytest.mark.parametrize("V,n,rows", [c for c in A.SHAPES if c[1] <= LIST])
def test_lists_equal_the_beam_kernels_bit_for_bit(dbg, V, n, rows, ts_on):
    """n entries are the list of a beam of width n - 1 (its N + 1 best): ids, counts and log-prob BITS.  n = 1 has no beam
    width of its own (N >= 1): it is compared with the first entry of width 1's list."""
    s = seeded(V, rows)
    cnt, tok, lp, _ = run_case(dbg, s, n, ts_on)
    N = max(n - 1, 1)
    bn, bt, bl = beam_lists(dbg, s, N, ts_on)
    assert np.array_equal(cnt, np.minimum(bn, n))
    for b in range(rows):
        k = int(cnt[b])
        assert np.array_equal(tok[b, :k], bt[b, :k]) and np.array_equal(bits(lp[b, :k]), bits(bl[b, :k])), b


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
@pytest.mark.parametrize("V,rows", [(1024, 10), (51865, 16)])
def test_a_request_for_16_begins_with_every_smaller_request(dbg, V, rows, ts_on):
    s = seeded(V, rows)
    c16, t16, l16, e16 = run_case(dbg, s, 16, ts_on)
    for k in (1, 2, 5, 9, 15):
        ck, tk, lk, ek = run_case(dbg, s, k, ts_on)
        assert np.array_equal(ck, np.minimum(c16, k))
        assert np.array_equal(tk, t16[:, :k]) and np.array_equal(bits(lk), bits(l16[:, :k]))
        assert np.array_equal(bits(ek), bits(e16))


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
def test_a_rows_bits_do_not_depend_on_the_group(dbg, ts_on):
    """Rows alone, 5 rows, 17 rows, subsets and permutations of the 128 return what those rows returned among 128: ids,
    counts, log-prob bits and entropy bits."""
    V, n, rows = 1024, 8, 128
    s = seeded(V, rows)
    c0, t0, l0, e0 = run_case(dbg, s, n, ts_on)
    g = np.random.default_rng(5)
    picks = [np.array([0]), np.array([127]), np.array([3]), np.arange(5), np.arange(40, 57), g.permutation(128)[:17], g.permutation(128),
             np.arange(127, -1, -1)[:64]]
    for idx in picks:
        c, t, l, e = run_case(dbg, s, n, ts_on, rows=idx)
        assert np.array_equal(c, c0[idx]) and np.array_equal(t, t0[idx]), idx
        assert np.array_equal(bits(l), bits(l0[idx])) and np.array_equal(bits(e), bits(e0[idx])), idx


def test_short_lists_empty_rows_and_what_is_written(dbg):
    """Fewer admissible ids than n, an empty admissible set, a suppressed id however large; the pads are written and the nullable
    outputs may be absent."""
    V, n = 1030, 6
    few = np.full((4, V), -np.inf, np.float32)
    few[0, [7, 3]] = 1.0                      # two equal values: the lower id first
    few[1, [900, 20, 21]] = (2.0, 0.5, 0.5)
    few[2, 5] = 40.0                          # suppressed below: nothing is left
    few[3, [5, 1029]] = (40.0, -3.0)          # the suppressed id does not enter, however large
    cnt, tok, lp, ent = run(dbg, few, n, [5], None, V - 124)
    assert list(cnt) == [2, 3, 0, 1]
    check_pads(cnt, tok, lp)
    assert list(tok[0, :2]) == [3, 7] and list(tok[1, :3]) == [900, 20, 21] and tok[3, 0] == 1029
    ref = [A.alternatives_np(few[b], n, [5]) for b in range(4)]
    _, want_lp, _, want_ent = A.packed(ref, n)
    assert np.abs(lp - want_lp).max() <= 2e-4 and np.abs(ent - want_ent).max() <= 2e-4
    assert bits(ent)[2] == 0 and bits(lp)[3, 0] == 0 and abs(float(ent[3])) <= 1e-6   # empty A: entropy +0; one id: log-prob 0
    # the nullable outputs absent: the lists are the same
    _, tok2, lp2, _ = run(dbg, few, n, [5], None, V - 124, counts=False, entropy=False)
    assert np.array_equal(tok2, tok) and np.array_equal(bits(lp2), bits(lp))


def test_bad_arguments_launch_nothing(dbg):
    lg = np.zeros((2, 64), np.float32)
    for n in (0, 17, -1):
        tok = np.full((2, 17), SENT_I, np.int32)
        lp = np.full((2, 17), SENT_F, np.float32)
        st = dbg.lib.wmdbg_alternatives(dbg.handle, _p(lg), 2, 64, n, None, 0, None, 0, None, _p(tok), _p(lp), None)
        assert st == 1 and np.all(tok == SENT_I) and np.all(lp == SENT_F)
    tok = np.full((2, 4), SENT_I, np.int32)
    lp = np.full((2, 4), SENT_F, np.float32)
    assert dbg.lib.wmdbg_alternatives(dbg.handle, _p(lg), 2, 64, 4, None, 0, None, 0, None, None, _p(lp), None) == 1
    assert dbg.lib.wmdbg_alternatives(dbg.handle, _p(lg), 2, 64, 4, None, 0, None, 0, None, _p(tok), None, None) == 1
    assert dbg.lib.wmdbg_alternatives(dbg.handle, _p(lg), 129, 64, 4, None, 0, None, 0, None, _p(tok), _p(lp), None) == 1
