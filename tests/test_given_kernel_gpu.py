"""Kernel-level tests of the given-tokens kernel (csrc/given.hip; wm_set_given_tokens) through the debug
hook wmdbg_decode_close_given: one decode position's logits launch, the given-tokens launch and the close, against the f64
restatement of tests/given_ref.py over the launch's OWN stored logits row, and bit for bit against the same step without the
launch (wmdbg_decode_close) wherever the kernel must change nothing.

The hook computes its logits itself (LayerNorm-folded GEMV of K = 64 over a seeded embedding), so the rows are this file's, not
alt_ref.seeded_rows': the timestamp ranges follow that file's recipe by row (an empty text range, an empty timestamp range, a
narrow text range, two wide ones) and are placed on the CPU, from the f64 reference logits, so that every finite sum-rule gap
is at least 0.25; the test then asserts |gap| >= alt_ref.MIN_SUM_RULE_GAP on the launch's own logits, so f32 and f64 agree on
`forced` and no row is skipped.  Log-probs: 1e-4 absolute against f64, the project's gate for this quantity
(tests/test_sampling_rules_gpu.py); -inf exactly where the restatement says so; tokens exact."""
import ctypes
import functools
import types

import numpy as np
import pytest

import alt_ref as A
import given_ref as G
import test_decode_step_kernels_gpu as DS
from test_decode_step_kernels_gpu import Step, bits, dbg, run_step   # noqa: F401 (dbg: fixture)
from test_sampling_rules_kernel_gpu import same_step

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
POOL, K = 128, 64
POS, N_PROMPT = 3, 2        # generated index 2
HIST0 = [3, 0, 0, -1]
VARIANTS = ("winner", "text", "timestamp", "bad_text", "bad_timestamp", "last")


@pytest.fixture(scope="module")
def hook(dbg):
    fn = dbg.lib.wmdbg_decode_close_given
    fn.argtypes = [vp, ctypes.POINTER(Step), vp, ip, ctypes.c_float, ctypes.c_float, vp, vp, vp]
    fn.restype = ip
    return fn


@functools.lru_cache(maxsize=None)
def world(V):
    """Operands of one vocabulary (never modified), as test_decode_step_kernels_gpu.world has them, for 128 rows: ts_begin =
    V - 124 (alt_ref's), eot ten ids below it, a suppress list with text ids and timestamps, and the f64 reference logits."""
    g = np.random.default_rng(7 * V + K)
    w = types.SimpleNamespace(V=V, ts_begin=V - 124, eot=V - 134, K=K)
    w.x = (g.standard_normal((POOL, K)) * (0.5 + np.arange(POOL) / POOL)[:, None] + 0.7).astype(np.float32)
    w.g = (1 + 0.1 * g.standard_normal(K)).astype(np.float32)
    w.beta = (0.1 * g.standard_normal(K)).astype(np.float32)
    emb = g.standard_normal((V, K)) * (2.0 / np.sqrt(K)) + np.linspace(-0.02, 0.02, K)[None, :] + np.linspace(-0.01, 0.01, V)[:, None]
    w.emb = DS.bf(emb)
    w.pemb = (g.standard_normal((448, K)) * 0.3 + 1.0).astype(np.float32)
    w.ref = DS.bf(DS.layer_norm64(w.x, w.g, w.beta)).astype(np.float64) @ w.emb.astype(np.float64).T
    sup = np.unique(np.concatenate([g.integers(0, w.ts_begin, 14), w.ts_begin + g.integers(0, 124, 6), [w.ts_begin - 3]]))
    w.suppress = tuple(int(s) for s in sup)
    # timestamps lifted so that the wide rows' gaps centre on 0: both decisions of the sum rule occur
    ok = np.ones(V, bool)
    ok[list(w.suppress)] = False
    tsb = w.ts_begin
    w.bias = np.zeros(V, np.float32)
    w.bias[tsb:] = np.median([w.ref[p, :tsb][ok[:tsb]].max() - DS.lse64(w.ref[p, tsb + 30:][ok[tsb + 30:]]) for p in range(POOL)])
    w.rng, w.gap = np.zeros((POOL, 4), np.int32), np.zeros(POOL)
    ref = w.ref + w.bias.astype(np.float64)
    for b in range(POOL):
        kind = (b + 3) % 5
        for lo in range(tsb + (7 * b) % 60, V):
            r4 = [(0, 0, tsb, tsb + 21), (0, tsb, lo, lo), (tsb - 10, tsb, lo, V), (0, tsb, lo, V), (0, tsb, lo, V)][kind]
            gap = A.admissible(ref[b], w.suppress, r4)[1]
            if not np.isfinite(gap) or abs(gap) >= 0.25:
                break
        else:
            raise AssertionError("no range of row %d is away from a tie" % b)
        w.rng[b], w.gap[b] = r4, gap
    return w


def run_given(dbg, hook, w, rows, given, rule=(0, 1.0, 0.0), **kw):
    """run_step with wmdbg_decode_close_given in the place of wmdbg_decode_close; r.keys: the rows' keys and winner values"""
    nt = (w.V + 15) // 16
    keys = types.SimpleNamespace(tilemax=np.zeros((len(rows), nt), np.uint64), key_ts=np.zeros((len(rows), nt), np.uint64),
                                 win=np.zeros((len(rows), nt, 2), np.float32))
    g = None if given is None else np.ascontiguousarray(given, np.int32)

    def close(handle, step):
        return hook(handle, step, DS.P(g), rule[0], rule[1], rule[2], DS.P(keys.tilemax), DS.P(keys.key_ts), DS.P(keys.win))
    stand_in = types.SimpleNamespace(handle=dbg.handle, lib=types.SimpleNamespace(wmdbg_decode_close=close, wm_last_error=dbg.lib.wm_last_error))
    r = run_step(stand_in, w, rows, **kw)
    r.keys = keys
    return r


def step_kw(w, rows, ts_on, **more):
    kw = dict(pos=POS, n_prompt=N_PROMPT, bias=w.bias, fallback=w.eot, suppress=w.suppress, xm=dict(T=0.0), **more)
    if ts_on:
        kw["ts"] = dict(mode=2, rng=w.rng[rows], hist=np.tile(HIST0, (len(rows), 1)))
    return kw


def pick(g, lo, hi, w, want_suppressed=False):
    """a seeded id of [lo, hi) that is (not) suppressed; None when there is none"""
    ids = [i for i in range(lo, hi) if (i in w.suppress) == want_suppressed]
    return int(ids[g.integers(0, len(ids))]) if ids else None


def variant_tokens(w, rows, base_tok):
    """per variant the id every row is given (none skipped): its own winner; a text id of its range; a timestamp of its range;
    a text id and a timestamp that are not admissible (suppressed, or outside the range); V - 1"""
    g = np.random.default_rng(w.V + len(rows))
    tsb, V = w.ts_begin, w.V
    out = {v: np.zeros(len(rows), np.int32) for v in VARIANTS}
    for j, b in enumerate(rows):
        tl, th, sl, sh = (int(x) for x in w.rng[b])
        out["winner"][j] = base_tok[j]
        t = pick(g, tl, th, w)
        out["text"][j] = t if t is not None else pick(g, 0, tsb, w)
        t = pick(g, sl, sh, w)
        out["timestamp"][j] = t if t is not None else pick(g, tsb, V, w)
        out["bad_text"][j] = pick(g, 0, tl, w) if (j % 2 and tl > 0) else pick(g, 0, tsb, w, want_suppressed=True)
        out["bad_timestamp"][j] = pick(g, tsb, sl, w) if (sl > tsb and j % 3) else pick(g, tsb, V, w, want_suppressed=True)
        out["last"][j] = V - 1
    return out


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
@pytest.mark.parametrize("V,B", G.SHAPES)
def test_every_row_given_every_kind_of_token(dbg, hook, V, B, ts_on):
    w = world(V)
    rows = np.arange(B)
    kw = step_kw(w, rows, ts_on)
    base = run_step(dbg, w, rows, **kw)
    none = run_given(dbg, hook, w, rows, None, **kw)
    same_step(none, base)                                                    # the hook without a table is the plain step
    rng = [w.rng[b] if ts_on else None for b in rows]
    for b in range(B):                                                       # f32 and f64 agree on `forced`: no row is skipped
        gap = A.admissible(base.logits[b], w.suppress, rng[b])[1]
        assert gap is None or not np.isfinite(gap) or abs(gap) >= A.MIN_SUM_RULE_GAP, (b, gap)
    toks = variant_tokens(w, rows, base.tok)
    cases, worst = set(), 0.0
    for name in VARIANTS:
        tok = toks[name]
        r = run_given(dbg, hook, w, rows, tok, **kw)
        assert np.array_equal(bits(r.logits), bits(base.logits))
        assert np.array_equal(r.tok, tok), (name, np.flatnonzero(r.tok != tok)[:5])              # exactly the given id
        assert np.array_equal(r.seq[POS + 1], tok)
        DS.check_embedding(w, r, tok, POS)
        for b in range(B):
            e = G.given_np(r.logits[b], int(tok[b]), w.suppress, rng[b], w.ts_begin)
            assert e.touched
            cases.add(e.case)
            got = float(r.logprob[b])
            if e.logprob == -np.inf:
                assert got == -np.inf, (name, b, int(tok[b]), got)
            else:
                assert np.isfinite(got), (name, b, int(tok[b]), got, e.logprob)
                worst = max(worst, abs(got - e.logprob))
            if ts_on:
                hist, nxt = G.ts_advance_np(HIST0, int(tok[b]), w.ts_begin, w.eot, V)
                assert r.hist[b].tolist() == hist and r.rng[b].tolist() == nxt, (name, b)
        if name == "winner":   # token, log-prob bits, next embedding and rule state of the step without the launch
            same_step(r, base)
    print("V %d B %d ts %d: max |dlogprob| %.3g over %d finite cases; cases %s" % (V, B, ts_on, worst, len(cases), sorted(cases)))
    assert worst <= 1e-4
    if not ts_on:
        assert cases == {G.CASES[8]}
    elif B >= 6:
        assert cases == set(G.CASES[:8]), sorted(set(G.CASES[:8]) - cases)


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
def test_rows_the_kernel_must_not_touch(dbg, hook, ts_on):
    """rows with -1, rows that are done and a prompt position keep their keys and winner values byte for byte, and everything
    the close makes of them"""
    w = world(1024)
    B = 17
    rows = np.arange(B)
    done = np.zeros(B, np.int32)
    done[[2, 16]] = 1
    kw = step_kw(w, rows, ts_on, stop=dict(done=done, eot=w.eot, pad=w.eot))
    none = run_given(dbg, hook, w, rows, None, **kw)
    given = np.full(B, -1, np.int32)
    touched = [0, 2, 5, 16]                                                  # (2 and 16 are done)
    given[touched] = [11, 12, w.ts_begin + 40, 13]
    r = run_given(dbg, hook, w, rows, given, **kw)
    free = [b for b in range(B) if b not in (0, 5)]
    for name in ("tilemax", "key_ts", "win"):
        a, b_ = getattr(r.keys, name), getattr(none.keys, name)
        assert np.array_equal(a[free].view(np.uint8), b_[free].view(np.uint8)), name
    assert not np.array_equal(r.keys.tilemax[0], none.keys.tilemax[0])
    assert r.tok[0] == 11 and r.tok[5] == w.ts_begin + 40 and r.tok[2] == w.eot and r.tok[16] == w.eot
    for name in ("logprob", "x_next", "xb_next", "stats"):
        assert np.array_equal(bits(getattr(r, name))[free], bits(getattr(none, name))[free]), name
    assert np.array_equal(r.tok[free], none.tok[free]) and np.array_equal(r.done, none.done)
    # a prompt position: nothing at all changes
    kw = step_kw(w, rows, ts_on)
    kw.update(pos=0, n_prompt=3)
    seq = np.random.default_rng(3).integers(0, 900, (DS.N_CTX, B)).astype(np.int32)
    a = run_given(dbg, hook, w, rows, None, seq=seq, **kw)
    b_ = run_given(dbg, hook, w, rows, np.full(B, 5, np.int32), seq=seq, **kw)
    same_step(b_, a)
    for name in ("tilemax", "key_ts", "win"):
        assert np.array_equal(getattr(a.keys, name).view(np.uint8), getattr(b_.keys, name).view(np.uint8)), name


def test_a_rows_bits_do_not_depend_on_the_group(dbg, hook):
    """a row alone, subsets and a permutation of the 128 return what those rows returned among 128"""
    w = world(1024)
    rows = np.arange(POOL)
    kw = step_kw(w, rows, True)
    base = run_step(dbg, w, rows, **kw)
    toks = variant_tokens(w, rows, base.tok)
    g = np.random.default_rng(5)
    for name in ("text", "timestamp"):
        big = run_given(dbg, hook, w, rows, toks[name], **kw)
        for idx in (np.array([0]), np.array([127]), np.arange(40, 57), g.permutation(128)[:17], g.permutation(128)):
            r = run_given(dbg, hook, w, idx, toks[name][idx], **step_kw(w, idx, True))
            assert np.array_equal(r.tok, big.tok[idx])
            for out in ("logprob", "x_next", "xb_next"):
                assert np.array_equal(bits(getattr(r, out)), bits(getattr(big, out))[idx]), (name, out)
            assert np.array_equal(r.rng, big.rng[idx]) and np.array_equal(r.hist, big.hist[idx])


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
def test_a_given_row_overrides_a_draw_and_keeps_the_normaliser(dbg, hook, ts_on):
    """A sampled step's own tokens given back -- at the sampling temperature, with and without the sampling rules, and at
    temperature 0 -- give the sampled step's token and log-prob bits; another id's log-prob is the temperature-1 one."""
    w = world(1030)
    B = 6
    rows = np.arange(B)
    kw = step_kw(w, rows, ts_on)
    kw["xm"] = dict(T=0.7, seed=2 ** 40 + 9, chunk0=3)
    sampled = run_step(dbg, w, rows, **kw)
    greedy = run_step(dbg, w, rows, **step_kw(w, rows, ts_on))
    assert (sampled.tok != greedy.tok).any()
    for rule in ((0, 1.0, 0.0), (8, 0.9, 0.0)):
        r = run_given(dbg, hook, w, rows, sampled.tok, rule=rule, **kw)
        same_step(r, sampled)
    cold = run_given(dbg, hook, w, rows, sampled.tok, **step_kw(w, rows, ts_on))
    assert np.array_equal(cold.tok, sampled.tok) and np.array_equal(bits(cold.logprob), bits(sampled.logprob))
    assert np.array_equal(bits(cold.x_next), bits(sampled.x_next))
    other = variant_tokens(w, rows, greedy.tok)["text"]
    hot = run_given(dbg, hook, w, rows, other, rule=(8, 0.9, 0.0), **kw)
    cold = run_given(dbg, hook, w, rows, other, **step_kw(w, rows, ts_on))
    assert np.array_equal(hot.tok, other) and np.array_equal(bits(hot.logprob), bits(cold.logprob))


def test_bad_arguments_launch_nothing(dbg, hook):
    w = world(1030)
    rows = np.arange(3)
    nt = (w.V + 15) // 16
    for given, x_on in (([1, w.V, 2], 1), ([-2, 1, 1], 1), ([1, 1, 1], 0)):
        s = Step()
        tm = np.full((3, nt), 0x77, np.uint64)
        g = np.ascontiguousarray(given, np.int32)
        lg = np.full((3, w.V), -123.25, np.float32)
        tok = np.full(3, -7, np.int32)
        s.B, s.V, s.K, s.n_ctx, s.pos, s.n_prompt, s.x_on = 3, w.V, K, DS.N_CTX, POS, N_PROMPT, x_on
        s.logits, s.tok = DS.P(lg), DS.P(tok)
        rc = hook(dbg.handle, ctypes.byref(s), DS.P(g), 0, 1.0, 0.0, DS.P(tm), DS.P(tm), DS.P(np.zeros((3, nt, 2), np.float32)))
        assert rc == DS.WM_ERR_INVALID and np.all(tm == 0x77) and np.all(lg == np.float32(-123.25)) and np.all(tok == -7)
    s = Step()
    assert hook(dbg.handle, ctypes.byref(s), None, 0, 1.0, 0.0, None, None, None) == DS.WM_ERR_INVALID
    assert hook(dbg.handle, None, None, 0, 1.0, 0.0, DS.P(tm), DS.P(tm), DS.P(tm)) == DS.WM_ERR_INVALID
