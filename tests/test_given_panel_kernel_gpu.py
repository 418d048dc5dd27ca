"""Kernel-level tests of the given-panel kernels (csrc/given_panel.hip; wm_set_given_panel) through the
debug hook wmdbg_given_panel_round: one round -- stage, the hook's own logits launch, close, commit -- on caller-given state,
against the f64 restatement of tests/given_ref.py over the launch's OWN stored logits rows and the bookkeeping restatement of
tests/given_panel_ref.py.

Rows follow tests/test_given_kernel_gpu.py's recipe (its `world`: residual rows, LayerNorm, embedding, suppress list, the lifted
timestamps).  In a round the ranges of row (c, s >= 1) are not free -- they follow from the tokens in front of it -- so the
residual row of every slot is PLACED from the pool on the CPU, from the f64 reference logits, so that every finite sum-rule gap
under the slot's ranges is at least 0.25; the test then asserts |gap| >= alt_ref.MIN_SUM_RULE_GAP on the launch's own logits.
Log-probs: 1e-4 absolute against f64 (the gate of the given and alternatives kernel files); -inf exactly where the restatement
says so; everything else array_equal, over WHOLE buffers so that sentinels show what the kernels left alone."""
import ctypes

import numpy as np
import pytest

import alt_ref as A
import given_panel_ref as R
import given_ref as G
import test_decode_step_kernels_gpu as DS
from spec_ref import ts_advance
from test_decode_step_kernels_gpu import dbg   # noqa: F401 (dbg: fixture)
from test_given_kernel_gpu import K, POOL, world

pytestmark = pytest.mark.gpu

vp, i32 = ctypes.c_void_p, ctypes.c_int32
SHAPES = [(1, 2), (1, 8), (5, 3), (64, 2), (16, 8)]   # G x w
VARIANTS = ("winner", "text", "timestamp", "bad_text", "bad_timestamp", "last")
N_CTX, N_PROMPT, POS, MAX_NEW = 16, 2, 3, 12           # the round's first generated index: g0 = 2
G0 = POS + 1 - N_PROMPT
ROWS = 128
HIST0 = [3, 0, 0, -1]
SENT = -77


class Round(ctypes.Structure):
    """struct wmdbg_given_panel"""
    _fields_ = [(n, i32) for n in ("G", "w", "V", "K", "n_ctx", "pos", "n_prompt", "max_new", "first", "last")] + \
               [(n, vp) for n in ("x", "ln_g", "ln_b", "emb", "bias", "suppress")] + \
               [(n, i32) for n in ("n_suppress", "fallback_tok", "ts_mode", "ts_begin", "eot")] + \
               [(n, vp) for n in ("hist", "rng", "chist", "crng")] + \
               [(n, i32) for n in ("stop_on", "stop_eot", "pad_tok")] + \
               [("done", vp), ("budget", vp), ("live_rows", vp), ("n_live", i32), ("glens", vp), ("gtok", vp), ("stride", i32),
                ("seq", vp), ("logprob", vp), ("wtok", vp), ("wlp", vp), ("logits", vp), ("pos_out", i32)]


@pytest.fixture(scope="module")
def hook(dbg):
    fn = dbg.lib.wmdbg_given_panel_round
    fn.argtypes = [vp, ctypes.POINTER(Round)]
    fn.restype = ctypes.c_int
    return fn


def ranges_of(w, G_, wd, crng, tok, ts_on):
    """the rows' ranges [G * w][4] behind the committed ranges and the table's tokens (None without rules)"""
    if not ts_on:
        return None
    out = np.zeros((G_ * wd, 4), np.int32)
    for c in range(G_):
        hist = list(HIST0)
        out[c * wd] = crng[c]
        for s in range(1, wd):
            hist, r = ts_advance(hist, int(tok[c][G0 + s - 1]), w.ts_begin, w.eot, w.V)
            out[c * wd + s] = r
    return out


def place(w, r4, start):
    """a pool row whose f64 reference logits keep their distance from a sum-rule tie under the ranges r4"""
    for k in range(POOL):
        p = (start + k) % POOL
        gap = A.admissible(w.ref[p] + w.bias.astype(np.float64), w.suppress, r4)[1]
        if gap is None or not np.isfinite(gap) or abs(gap) >= 0.25:
            return p
    raise AssertionError("no pool row is away from a tie under %s" % (r4,))


def pick(g, lo, hi, w, suppressed=False):
    ids = [i for i in range(max(lo, 0), min(hi, w.V)) if (i in w.suppress) == suppressed]
    return int(ids[g.integers(0, len(ids))]) if ids else None


def build(w, G_, wd, variant, ts_on, seed):
    """slot by slot: the slot's ranges follow from the ids in front of it, its residual row is placed, its given id is the
    variant's.  Returns (pool rows [G * w], table tok [G][MAX_NEW], committed ranges [G][4])."""
    g = np.random.default_rng(seed)
    tsb, V = w.ts_begin, w.V
    rows = np.zeros(G_ * wd, np.int64)
    tok = g.integers(0, w.eot, (G_, MAX_NEW)).astype(np.int32)
    crng = np.zeros((G_, 4), np.int32)
    for c in range(G_):
        crng[c] = w.rng[(c * 7 + 1) % POOL]                       # the recipe's ranges by row, as the committed state
        hist, r4 = list(HIST0), tuple(int(x) for x in crng[c])
        for s in range(wd):
            b = c * wd + s
            p = place(w, r4 if ts_on else None, b * 3 + seed)
            rows[b] = p
            ref = w.ref[p] + w.bias.astype(np.float64)
            tl, th, sl, sh = r4 if ts_on else (0, V, 0, 0)
            if variant == "winner":
                ok = A.admissible(ref, w.suppress, r4 if ts_on else None)[0]
                t = int(np.argmax(np.where(ok, ref, -np.inf)))
            elif variant == "text":
                t = pick(g, tl, min(th, tsb) if ts_on else tsb, w)
                t = t if t is not None else pick(g, 0, tsb, w)
            elif variant == "timestamp":
                t = pick(g, sl, sh, w) if ts_on else None
                t = t if t is not None else pick(g, tsb, V, w)
            elif variant == "bad_text":
                t = pick(g, 0, tl, w) if (b % 2 and tl > 0 and ts_on) else pick(g, 0, tsb, w, suppressed=True)
            elif variant == "bad_timestamp":
                t = pick(g, tsb, sl, w) if (sl > tsb and b % 3 and ts_on) else pick(g, tsb, V, w, suppressed=True)
            else:
                t = V - 1
            tok[c, G0 + s] = t
            if ts_on:
                hist, r4 = ts_advance(hist, t, tsb, w.eot, V)
                r4 = tuple(int(x) for x in r4)
    return rows, tok, crng


def run_round(dbg, hook, w, G_, wd, rows, tok, lens, crng, ts_on, first=True, last=True, stop=None, seq_pos=None):
    """one hook call; every state buffer is sentinel-filled where the round has no business.  Returns (io arrays before, after)."""
    V = w.V
    st = dict(hist=np.full((ROWS, 4), 5, np.int32), rng=np.full((ROWS, 4), 7, np.int32), chist=np.full((ROWS, 4), 9, np.int32),
              crng=np.full((ROWS, 4), 11, np.int32), done=np.full(ROWS, SENT, np.int32), live_rows=np.full(ROWS, SENT, np.int32),
              seq=np.full((N_CTX + 1, G_), 1, np.int32), logprob=np.full((MAX_NEW, G_), -123.25, np.float32),
              wtok=np.full(ROWS, SENT, np.int32), wlp=np.full(ROWS, -321.5, np.float32))
    (st["hist"] if first else st["chist"])[:G_] = HIST0
    (st["rng"] if first else st["crng"])[:G_] = crng
    st["seq"][POS] = seq_pos if seq_pos is not None else 2
    budget = None
    if stop is not None:
        st["done"][:G_] = stop["done"]
        budget = None if stop.get("budget") is None else np.ascontiguousarray(stop["budget"], np.int32)
    before = {k: v.copy() for k, v in st.items()}
    logits = np.zeros((G_ * wd, V), np.float32)
    x = np.ascontiguousarray(w.x[rows])
    sup = np.ascontiguousarray(w.suppress, np.int32)
    lens_a, tok_a = np.ascontiguousarray(lens, np.int32), np.ascontiguousarray(tok, np.int32)
    io = Round()
    io.G, io.w, io.V, io.K, io.n_ctx, io.pos, io.n_prompt, io.max_new = G_, wd, V, K, N_CTX, POS, N_PROMPT, MAX_NEW
    io.first, io.last = int(first), int(last)
    io.x, io.ln_g, io.ln_b, io.emb, io.bias = DS.P(x), DS.P(w.g), DS.P(w.beta), DS.P(w.emb), DS.P(w.bias)
    io.suppress, io.n_suppress, io.fallback_tok = DS.P(sup), len(sup), w.eot
    io.ts_mode, io.ts_begin, io.eot = (2 if ts_on else 0), w.ts_begin, w.eot
    io.hist, io.rng, io.chist, io.crng = (DS.P(st[k]) for k in ("hist", "rng", "chist", "crng"))
    io.stop_on = int(stop is not None)
    io.stop_eot, io.pad_tok = (stop["eot"] if stop is not None else -1), w.eot
    io.done, io.budget, io.live_rows, io.n_live = DS.P(st["done"]), DS.P(budget), DS.P(st["live_rows"]), SENT
    io.glens, io.gtok, io.stride = DS.P(lens_a), DS.P(tok_a), MAX_NEW
    io.seq, io.logprob, io.wtok, io.wlp, io.logits = (DS.P(a) for a in (st["seq"], st["logprob"], st["wtok"], st["wlp"], logits))
    io.pos_out = SENT
    rc = hook(dbg.handle, ctypes.byref(io))
    assert rc == 0, DS.err_msg(dbg)
    st["logits"], st["n_live"], st["pos_out"] = logits, io.n_live, io.pos_out
    return before, st


def expected(w, G_, wd, before, tok, lens, ts_on, got, first, last, stop):
    """the restatement on the state the hook was given, with the close's own (wtok, wlp): every buffer the round may write"""
    ts = (w.ts_begin, w.eot, w.V) if ts_on else None
    st = dict(seq=before["seq"].tolist(), lens=[int(x) for x in lens], tok=[[int(t) for t in r] for r in tok],
              hist=before["hist"].tolist(), rng=before["rng"].tolist(), chist=before["chist"].tolist(), crng=before["crng"].tolist(),
              done=[int(d) if stop is not None else 0 for d in before["done"][:G_]], logprob=before["logprob"].tolist())
    rows = R.stage_round(st, G_, wd, G0, N_PROMPT, N_CTX, ts, w.eot, first)
    n_live, live = R.commit_round(st, G_, wd, G0, N_PROMPT, MAX_NEW, got["wtok"][:G_ * wd].tolist(), got["wlp"][:G_ * wd].tolist(),
                                  stop["eot"] if stop is not None else -1, None if stop is None else stop.get("budget"), w.eot, ts, last)
    exp = {k: v.copy() for k, v in before.items()}
    exp["seq"] = np.array(st["seq"], np.int32)
    exp["logprob"] = np.array(st["logprob"], np.float32)
    if ts_on:
        exp["rng"][:G_ * wd] = rows
        exp["chist"][:G_], exp["crng"][:G_] = st["chist"][:G_], st["crng"][:G_]
        if last:
            exp["hist"][:G_], exp["rng"][:G_] = st["chist"][:G_], st["crng"][:G_]
    if stop is not None:
        exp["done"][:G_] = st["done"]
        exp["live_rows"][:n_live] = live
    return exp, rows, n_live, st["pos"]


def check_state(exp, got, what):
    for name in ("seq", "hist", "rng", "chist", "crng", "done", "live_rows"):
        assert np.array_equal(got[name], exp[name]), (what, name)
    assert np.array_equal(DS.bits(got["logprob"]), DS.bits(exp["logprob"])), (what, "logprob")


def free_close(dbg, hook, w, G_, wd, rows, tok, crng, ts_on):
    """The same G * w residual rows closed WITHOUT a table: a round of G * w windows of width 1 whose committed ranges are the
    slots' own, so row b is closed under exactly the ranges slot b of the panel sees (the logits launch is the same launch: the
    same rows in the same order).  The table's winner ids are taken from THIS close, the launch's own choice: where it differs
    from the f64 reference's (a near-tie), tok is corrected in place and the ranges behind it follow; a window's slots settle
    front to back, so at most w passes.  Returns the settled free round."""
    n = G_ * wd
    for _ in range(wd + 1):
        rr = ranges_of(w, G_, wd, crng, tok, ts_on)
        _, free = run_round(dbg, hook, w, n, 1, rows, np.zeros((n, MAX_NEW), np.int32), [0] * n,
                            rr if ts_on else np.zeros((n, 4), np.int32), ts_on)
        own = free["wtok"][:n].reshape(G_, wd)
        if np.array_equal(own, tok[:, G0:G0 + wd]):
            return free
        tok[:, G0:G0 + wd] = own
    raise AssertionError("the winners did not settle")


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "ts_mode_2"])
@pytest.mark.parametrize("V", [1030, 1024])
@pytest.mark.parametrize("G_,wd", SHAPES)
def test_every_row_given_every_kind_of_token(dbg, hook, G_, wd, V, ts_on):
    w = world(V)
    lens = [MAX_NEW] * G_
    cases, worst, n_inf = set(), 0.0, 0
    for vi, variant in enumerate(VARIANTS):
        rows, tok, crng = build(w, G_, wd, variant, ts_on, seed=31 * vi + G_ + wd)
        free = None
        if variant == "winner":
            free = free_close(dbg, hook, w, G_, wd, rows, tok, crng, ts_on)
        before, got = run_round(dbg, hook, w, G_, wd, rows, tok, lens, crng, ts_on)
        rr = ranges_of(w, G_, wd, crng, tok, ts_on)
        given = np.array([tok[c, G0 + s] for c in range(G_) for s in range(wd)], np.int32)
        assert np.array_equal(got["wtok"][:G_ * wd], given), (variant, np.flatnonzero(got["wtok"][:G_ * wd] != given)[:5])
        assert np.all(got["wtok"][G_ * wd:] == SENT) and np.all(DS.bits(got["wlp"][G_ * wd:]) == DS.bits(np.float32(-321.5)))
        for b in range(G_ * wd):
            r4 = None if rr is None else rr[b]
            gap = A.admissible(got["logits"][b], w.suppress, r4)[1]
            assert gap is None or not np.isfinite(gap) or abs(gap) >= A.MIN_SUM_RULE_GAP, (variant, b, gap)
            e = G.given_np(got["logits"][b], int(given[b]), w.suppress, r4, w.ts_begin)
            assert e.touched
            cases.add(e.case)
            lp = float(got["wlp"][b])
            if e.logprob == -np.inf:
                assert lp == -np.inf, (variant, b, int(given[b]), lp)
                n_inf += 1
            else:
                assert np.isfinite(lp), (variant, b, int(given[b]), lp, e.logprob)
                worst = max(worst, abs(lp - e.logprob))
            if variant.startswith("bad"):
                assert lp == -np.inf, (variant, b)
        exp, rows_exp, n_live, pos = expected(w, G_, wd, before, tok, lens, ts_on, got, True, True, None)
        check_state(exp, got, variant)
        assert got["pos_out"] == pos == POS + wd and got["n_live"] == SENT
        if variant == "winner":   # every row closes as it does without a table: the same token and log-prob bits
            assert np.array_equal(got["wtok"][:G_ * wd], free["wtok"][:G_ * wd])
            assert np.array_equal(DS.bits(got["wlp"][:G_ * wd]), DS.bits(free["wlp"][:G_ * wd]))
            assert np.array_equal(DS.bits(got["logits"]), DS.bits(free["logits"]))
    print("G %d w %d V %d ts %d: max |dlogprob| %.3g, %d at -inf; cases %s" % (G_, wd, V, ts_on, worst, n_inf, sorted(cases)))
    assert worst <= 1e-4 and n_inf >= 2 * G_ * wd
    if not ts_on:
        assert cases == {G.CASES[8]}
    elif G_ * wd >= 15:
        assert cases == set(G.CASES[:8]), sorted(set(G.CASES[:8]) - cases)


def commit_case(w, G_, wd, seed):
    """a seeded state for a commit: done flags, budgets, a table with eot here and there; the classes the restatement sees"""
    g = np.random.default_rng(seed)
    mode = seed % 5
    done = (g.random(G_) < (1.0 if mode == 0 else 0.25)).astype(np.int32)
    budget = g.integers(G0 + 1, MAX_NEW + 1, G_).astype(np.int32)
    tok = g.integers(0, w.eot, (G_, MAX_NEW)).astype(np.int32)
    if mode == 1:                                  # everybody stops: an eot in every window's panel
        tok[np.arange(G_), G0 + g.integers(0, wd, G_)] = w.eot
    elif mode == 2:
        tok[g.random(G_) < 0.5, G0] = w.eot         # at row 0
    elif mode == 3:
        tok[g.random(G_) < 0.5, G0 + wd - 1] = w.eot   # at row w - 1
    else:
        hit = g.random((G_, MAX_NEW)) < 0.1
        tok[hit] = w.eot
    return done, budget, tok


def classes(G_, wd, done, budget, tok, eot):
    """what the restatement alone says of a case"""
    out = set()
    if done.all():
        out.add("nobody live")
    stops = []
    for c in range(G_):
        if done[c]:
            continue
        at = [i for i in range(wd) if tok[c, G0 + i] == eot or G0 + i + 1 >= budget[c]]
        stops.append(at[0] if at else None)
        if at and tok[c, G0 + at[0]] != eot:       # the budget ends at a row of this panel
            out.add("budget inside")
    if stops and all(s is not None for s in stops):
        out.add("everybody stops")
    if any(s == 0 for s in stops):
        out.add("stop at row 0")
    if any(s == wd - 1 for s in stops):
        out.add("stop at row w - 1")
    return out


@pytest.mark.parametrize("G_,wd", SHAPES)
def test_forty_seeded_commits(dbg, hook, G_, wd):
    w = world(1024)
    seen = set()
    for k in range(40):
        seed = 1000 * G_ + 40 * wd + k
        ts_on, first, last = bool(k % 2), k % 3 != 1, k % 4 != 2
        done, budget, tok = commit_case(w, G_, wd, seed)
        seen |= classes(G_, wd, done, budget, tok, w.eot)
        lens = [MAX_NEW] * G_
        crng = np.array([w.rng[(c + k) % POOL] for c in range(G_)], np.int32)
        rows = (np.arange(G_ * wd) * 5 + k) % POOL
        stop = dict(done=done, eot=w.eot, budget=budget.tolist())
        before, got = run_round(dbg, hook, w, G_, wd, rows, tok, lens, crng, ts_on, first=first, last=last, stop=stop)
        exp, _, n_live, pos = expected(w, G_, wd, before, tok, lens, ts_on, got, first, last, stop)
        check_state(exp, got, (k, ts_on, first, last))
        assert got["n_live"] == n_live and got["pos_out"] == pos
        if not ts_on:   # without rules every id in the vocabulary's text is admissible or -inf: the close keeps the table's id
            given = np.array([tok[c, G0 + s] for c in range(G_) for s in range(wd)], np.int32)
            assert np.array_equal(got["wtok"][:G_ * wd], given)
    want = {"nobody live", "everybody stops", "stop at row 0", "stop at row w - 1", "budget inside"}
    assert seen == want, sorted(want - seen)


def test_bad_arguments_launch_nothing(dbg, hook):
    w = world(1030)
    rows, tok, crng = build(w, 2, 3, "text", True, 1)
    for change in (dict(w=9), dict(pos=N_PROMPT - 1), dict(pos=N_CTX - 3), dict(ts_mode=1), dict(G=65, w=2)):
        io = Round()
        io.G, io.w, io.V, io.K, io.n_ctx, io.pos, io.n_prompt, io.max_new, io.stride = 2, 3, w.V, K, N_CTX, POS, N_PROMPT, MAX_NEW, MAX_NEW
        for k, v in change.items():
            setattr(io, k, v)
        assert hook(dbg.handle, ctypes.byref(io)) == DS.WM_ERR_INVALID, change
    assert hook(dbg.handle, None) == DS.WM_ERR_INVALID
