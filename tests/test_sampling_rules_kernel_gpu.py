"""Kernel-level tests of the sampling rules (csrc/sample_trunc.hip; wm_set_sampling_rules) through the
debug hooks: wmdbg_sample_truncate -- the truncation kernel alone on the rows of tests/sampling_ref.py, against the f64
restatement there -- and wmdbg_decode_close_trunc -- a whole decode position's logits launch, truncation and close, against
wmdbg_decode_close on the same operands (bit for bit where the rules keep everything or one id).

Exactness: top_k cases are exact.  A top_p / min_p case is exact where the restatement's slack exceeds 1e-4; inside it any
count whose threshold lies within 1e-4 of the restatement's is accepted (f32 exp of arguments in [-88, 0] and the 2^-40
quantisation move a mass by two orders less).  The launches checked against the restatement are sampling_ref.checked_cases,
and tests/test_sampling_rules_cpu.py caps the share of near-threshold rows among exactly those at 5 %."""
import ctypes
import functools
import types

import numpy as np
import pytest

import sampling_ref as S
import test_decode_step_kernels_gpu as DS
from test_decode_step_kernels_gpu import Step, bits, dbg, run_step, sum_rule_inputs, world   # noqa: F401 (dbg: fixture)
from test_transcribe_options_cpu import gumbel_np

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
SEED = 2 ** 40 + 7


@pytest.fixture(scope="module")
def hook(dbg):
    fn = dbg.lib.wmdbg_sample_truncate
    fn.argtypes = [vp, vp, ip, ip, vp, ip, vp, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64, vp, ip, ip, ctypes.c_float,
                   ctypes.c_float, vp, vp, vp]
    dbg.lib.wmdbg_decode_close_trunc.argtypes = [vp, ctypes.POINTER(Step), ip, ctypes.c_float, ctypes.c_float]
    return fn


@functools.lru_cache(maxsize=None)
def pool(V):
    """The rows of one vocabulary; each row's order and masses (sampling_ref.case_reference) and its noise are computed once."""
    inp = S.hook_inputs(V)
    return types.SimpleNamespace(inp=inp, cache={}, noise={})


def noise(p, row, gi):
    key = (row, gi)
    if key not in p.noise:
        p.noise[key] = gumbel_np(SEED, int(p.inp.sample_ids[row]), gi, np.arange(p.inp.V))
    return p.noise[key]


def truncate(hook, dbg, p, rows, rule, gi, T=1.0, with_rng=True):
    inp = p.inp
    rows = np.asarray(rows)
    lg = np.ascontiguousarray(inp.logits[rows])
    rng = np.ascontiguousarray(inp.rng[rows]) if with_rng else None
    sup = np.asarray(inp.suppress, np.int32)
    ids = np.ascontiguousarray(inp.sample_ids[rows])
    out = [np.full(rows.size, -7, np.int32) for _ in range(3)]
    rc = hook(dbg.handle, DS.P(lg), rows.size, inp.V, DS.P(sup), sup.size, DS.P(rng), inp.ts_begin, T, SEED, DS.P(ids), gi,
              rule[0], rule[1], rule[2], DS.P(out[0]), DS.P(out[1]), DS.P(out[2]))
    assert rc == 0, DS.err_msg(dbg)
    return out


def check_row(p, row, rule, gi, got, detail, inv_T=1.0, draw=True):
    """One row's (kept_n, cut_tok, tok) against the restatement `detail`; returns whether the row was inside the slack."""
    kn, ct, tk = (int(x) for x in got)
    d = detail
    if d.count == 0:
        assert (kn, ct, tk) == (0, -1, -1), (row, rule, got)
        return False
    exact = (rule[1] >= 1.0 and rule[2] <= 0.0) or d.slack > S.TOL
    if exact:
        assert kn == d.count, (row, p.inp.kinds[row], rule, kn, d.count, d.slack)
    else:
        assert kn in d.accept, (row, p.inp.kinds[row], rule, kn, sorted(d.accept), d.slack)
    assert ct == int(d.ids[kn - 1]), (row, rule, ct, int(d.ids[kn - 1]))          # ties: the lowest ids
    keep = d.ids[:kn]
    assert tk in keep, (row, rule, tk)
    if draw:
        g = noise(p, row, gi)[keep]
        sc = p.inp.logits[row][keep].astype(np.float64) * float(np.float32(inv_T)) + g
        at = int(np.flatnonzero(keep == tk)[0])
        best = int(np.argmax(sc))
        assert sc[best] - sc[at] <= 1e-4 * max(1.0, abs(g[at]), abs(g[best])), (row, rule, tk, int(keep[best]))
    return not exact


def launch_and_check(hook, dbg, p, case, gi, draw_rows=None):
    """One case of sampling_ref.checked_cases: the launch, and every row against the restatement.  Returns the rows' outputs
    and how many rows were inside the slack."""
    T, with_rng, rule, rows = case
    inv_T = float(np.float32(1.0 / T))
    got = truncate(hook, dbg, p, rows, rule, gi, T=T, with_rng=with_rng)
    ref = S.case_reference(p.inp, T, with_rng, rule, rows, p.cache)
    near = 0
    for j, row in enumerate(rows):
        near += check_row(p, row, rule, gi, [o[j] for o in got], ref[j], inv_T=inv_T, draw=draw_rows is None or row in draw_rows)
    return got, near


N_POOL_CASES = len(S.RULES)


@pytest.mark.parametrize("k", range(N_POOL_CASES))
@pytest.mark.parametrize("V", sorted(S.GEOM))
def test_the_whole_pool_under_every_rule_set(hook, dbg, V, k):
    """All 128 rows (every kind, wide and narrow ranges) in one launch under rule set k; generated index 0 (the first-position
    bitmap) and 3 alternate.  (At 51 865 ids the draw is restated for the first 40 rows: the noise of a row is 51 865 Philox words.)"""
    p = pool(V)
    case = S.checked_cases(V)[k]
    assert case[0] == 1.0 and case[1] and len(case[3]) == S.POOL_ROWS
    _, near = launch_and_check(hook, dbg, p, case, 0 if k % 2 else 3, draw_rows=None if V < 51865 else range(40))
    print("V %d rule %s: %d of %d rows inside the slack" % (V, case[2], near, S.POOL_ROWS))


@pytest.mark.parametrize("V", sorted(S.GEOM))
def test_row_subsets_and_permutations(hook, dbg, V):
    """A row alone, 5 rows and a permutation of 17 return what those rows returned among 128: equal outputs, not merely
    acceptable ones."""
    p = pool(V)
    allr = list(range(S.POOL_ROWS))
    for rule in [r for r in S.rules_for(V) if r in ((50, 1.0, 0.0), (0, 0.9, 0.0), (50, 0.9, 0.05))]:
        big = truncate(hook, dbg, p, allr, rule, 2)
        perm = [S.SUB17[i] for i in np.random.default_rng(V).permutation(17)]
        for rows in ([3], [70], [0, 9, 34, 66, 127], perm):
            small = truncate(hook, dbg, p, rows, rule, 2)
            for a, b in zip(small, big):
                assert np.array_equal(a, b[rows]), (rule, rows, a, b[rows])


@pytest.mark.parametrize("V", sorted(S.GEOM))
def test_temperature_two_and_no_timestamp_rules(hook, dbg, V):
    """T = 2 flattens the rows (top_k = 1000 and V + 7 keep up to the whole vocabulary; the equal rows' nucleus is 90 % of it),
    and a call without timestamp rules: every id that is not suppressed is admissible."""
    p = pool(V)
    extra = S.checked_cases(V)[N_POOL_CASES:]
    assert len(extra) == 6 and all(c[3] == S.SUB17 for c in extra)
    for case in extra:
        launch_and_check(hook, dbg, p, case, 1)


# ------------------------------------------------------------------------------------------------- the whole step
def run_trunc(dbg, w, rows, rule, **kw):
    """run_step with wmdbg_decode_close_trunc in the place of wmdbg_decode_close."""
    fn = dbg.lib.wmdbg_decode_close_trunc

    def close(handle, step):
        return fn(handle, step, rule[0], rule[1], rule[2])
    stand_in = types.SimpleNamespace(handle=dbg.handle, lib=types.SimpleNamespace(wmdbg_decode_close=close, wm_last_error=dbg.lib.wm_last_error))
    return run_step(stand_in, w, rows, **kw)


def same_step(a, b, names=("logits", "logprob", "nospeech", "x_next", "xb_next", "stats")):
    for name in names:
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.array_equal(a.tok, b.tok) and np.array_equal(a.seq, b.seq) and a.logprob_written == b.logprob_written
    for name in ("rng", "hist", "done", "live"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), name
    assert a.n_live == b.n_live


@pytest.mark.parametrize("ts_on", [True, False], ids=["rules", "norules"])
@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("geom", ["small64", "production"])
def test_the_step_with_everything_kept_or_one_id_kept(hook, dbg, geom, B, ts_on):
    """(0, 1, 0) and top_k = V + 7 equal the sampled wmdbg_decode_close in every output, bit for bit -- the second-stage draw
    reproduces the fused one, and the hand-over leaves the close's decision, log-prob, timestamp-rule advance, stop state and
    embedding alone.  top_k = 1 at T = 1 equals the T = 0 close: token, log-prob, next embedding."""
    w = world(geom)
    rows, bias, rng, special = sum_rule_inputs(w, B)
    done = np.zeros(B, np.int32)
    done[B // 2] = 1
    kw = dict(bias=bias, fallback=w.eot, suppress=(2, 9, w.ts_begin + 3), stop=dict(done=done, eot=w.eot, pad=w.eot))
    if ts_on:
        kw["ts"] = dict(mode=2, rng=rng, hist=np.tile([3, 0, 0, -1], (B, 1)))
    for seed in (5, 2 ** 63 + 11):
        xm = dict(T=1.0, seed=seed, chunk0=7)
        plain = run_step(dbg, w, rows, xm=xm, **kw)
        same_step(run_trunc(dbg, w, rows, (0, 1.0, 0.0), xm=xm, **kw), plain)
        same_step(run_trunc(dbg, w, rows, (w.V + 7, 1.0, 0.0), xm=xm, **kw), plain)
        greedy = run_step(dbg, w, rows, xm=dict(T=0.0, seed=seed, chunk0=7), **kw)
        one = run_trunc(dbg, w, rows, (1, 1.0, 0.0), xm=xm, **kw)
        same_step(one, greedy)
        assert (plain.tok != greedy.tok).any()          # (the sampled step is not the greedy one: the comparisons say something)
    # the rules are ignored at temperature 0
    same_step(run_trunc(dbg, w, rows, (3, 0.5, 0.1), xm=dict(T=0.0, seed=1, chunk0=7), **kw), greedy)


@pytest.mark.parametrize("geom", ["small64", "production"])
def test_the_steps_token_lies_in_the_kept_set_of_its_own_logits(hook, dbg, geom):
    """(8, 1, 0) and (50, 0.9, 0.05) on a step with timestamp rules: the token is in the restatement's kept set of the step's
    own stored logits, and the log-prob is the untruncated filtered one (the sampled step's normaliser)."""
    w = world(geom)
    B = 16
    rows, bias, rng, special = sum_rule_inputs(w, B)
    sup = (2, 9, w.ts_begin + 3)
    kw = dict(bias=bias, fallback=w.eot, suppress=sup, ts=dict(mode=2, rng=rng, hist=np.tile([3, 0, 0, -1], (B, 1))))
    xm = dict(T=1.0, seed=77, chunk0=0)
    plain = run_step(dbg, w, rows, xm=xm, **kw)
    for rule in ((8, 1.0, 0.0), (50, 0.9, 0.05)):
        r = run_trunc(dbg, w, rows, rule, xm=xm, **kw)
        assert np.array_equal(bits(r.logits), bits(plain.logits))
        for b in range(B):
            adm, forced, gap = S.admissible_set(r.logits[b], w.V, sup, rng[b])
            d = S.kept_detail(r.logits[b], adm, 1.0, *rule)
            if d.count == 0:
                assert r.tok[b] == w.eot and r.logprob[b] == -np.inf
                continue
            assert abs(gap) > 1e-3                                           # (the inputs' sum rule is away from its tie)
            hi = max(d.accept) if d.slack <= S.TOL else d.count
            assert int(r.tok[b]) in d.ids[:hi], (rule, b, int(r.tok[b]))
            v = r.logits[b].astype(np.float64)
            lp = v[r.tok[b]] - (v[adm].max() + np.log(np.exp(v[adm] - v[adm].max()).sum()))
            assert abs(lp - float(r.logprob[b])) <= 1e-4, (rule, b, lp, float(r.logprob[b]))
