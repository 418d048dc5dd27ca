"""CPU tests of given panels (wm_set_given_panel): the plan (tx_plan.cpp wm_given_panel_plan through its
wmdbg_ mirror) against the restatement in tests/given_panel_ref.py over a full product and seeded cases; the round restatement
on hand-worked cases; the binding (Context.set_given_panel, score_given(form=)) on a stand-in library."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import given_panel_ref as R
import test_binding_calls_cpu as BC
from test_binding_calls_cpu import P3, RAGGED
from test_given_cpu import given_ctx, names, windows

B = importlib.import_module("openai_whisper_coreml_amd.binding")
IP = ctypes.POINTER(ctypes.c_int32)
SERVED_BITS = R.B_GIVEN | R.B_X


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_given_panel_plan.argtypes = [ctypes.c_int, ctypes.c_int, IP, IP] + [ctypes.c_int] * 3 + [ctypes.c_uint32, IP]
    lib.wmdbg_given_panel_plan.restype = ctypes.c_int
    lib.wmdbg_given_panel_plan_batch.argtypes = [ctypes.c_int, ctypes.c_int, IP, IP]
    lib.wmdbg_given_panel_plan_batch.restype = ctypes.c_int
    return lib


def batch(lib, G, width, lens, bud, has_bud, max_new, P, n_ctx, bits):
    n, g_max = lens.shape
    tab = np.zeros((n, 8 + 2 * g_max), np.int32)
    for k, col in enumerate((G, width, max_new, P, n_ctx, bits, has_bud)):
        tab[:, k] = col
    tab[:, 8:8 + g_max] = lens
    tab[:, 8 + g_max:] = bud
    out = np.full((n, 4), -7, np.int32)
    assert lib.wmdbg_given_panel_plan_batch(n, g_max, tab.ctypes.data_as(IP), out.ctypes.data_as(IP)) == 0
    return out


# ---------------------------------------------------------------- the plan
def test_the_two_restatements_of_the_plan_agree():
    g = np.random.default_rng(3)
    n = 400
    G = g.integers(1, 4, n)
    lens, bud = g.integers(0, 6, (n, 3)), g.integers(1, 6, (n, 3))
    width, max_new, has_bud = g.integers(1, 5, n), g.integers(1, 6, n), g.integers(0, 2, n)
    P, n_ctx = g.integers(1, 4, n), g.integers(4, 9, n)
    bits = np.where(g.random(n) < 0.8, SERVED_BITS, g.integers(0, 1 << 14, n))
    tab = R.plan_table(G, width, lens, bud, has_bud, max_new, P, n_ctx, bits)
    for i in range(n):
        one = R.plan(int(G[i]), int(width[i]), lens[i, :G[i]].tolist(), bud[i, :G[i]].tolist() if has_bud[i] else None, int(max_new[i]),
                     int(P[i]), int(n_ctx[i]), int(bits[i]))
        assert tuple(tab[i]) == one, i


def test_the_plan_over_the_full_product(lib):
    """G <= 3, lens 0 .. 5, budgets 1 .. 5 (and none), max_new <= 5, width <= 4, served mode: a roomy context, and a short one that
    cuts the phase."""
    total = served = cut = 0
    for G in (1, 2, 3):
        rows = np.array(list(itertools.product(range(6), repeat=G)), np.int32)            # lens
        buds = np.array(list(itertools.product(range(1, 6), repeat=G)), np.int32)
        lb = np.array([(i, j) for i in range(len(rows)) for j in range(len(buds))])
        for max_new, width, has_bud, n_ctx in itertools.product(range(1, 6), range(1, 5), (0, 1), (64, 6)):
            if not has_bud:
                lens, bud = rows, np.zeros_like(rows)
            else:
                lens, bud = rows[lb[:, 0]], buds[lb[:, 1]]
            n = len(lens)
            pad = lambda a: np.pad(a, ((0, 0), (0, 3 - G)))
            args = (np.full(n, G), np.full(n, width), pad(lens), pad(bud), np.full(n, has_bud), np.full(n, max_new), np.full(n, 3),
                    np.full(n, n_ctx), np.full(n, SERVED_BITS))
            want = R.plan_table(*args)
            got = batch(lib, *args)
            assert np.array_equal(got, want), (G, max_new, width, has_bud, n_ctx)
            total += n
            served += int((want[:, 0] == R.SERVED).sum())
            cut += int(((want[:, 0] == R.SERVED) & (want[:, 2] == n_ctx - 3) & (max_new > n_ctx - 3)).sum())
    print("plan product: %d cases, %d served, %d cut by the context" % (total, served, cut))
    assert total > 500000 and served > 10000 and cut > 0


def test_the_plan_on_seeded_groups_and_every_reason(lib):
    """Up to G = 128 and width 8, every mode bit: each reason of "Served groups" occurs, and its count is the restatement's."""
    g = np.random.default_rng(17)
    n = 6000
    G = g.integers(1, 129, n)
    width = g.integers(1, 9, n)
    max_new = g.integers(1, 30, n)
    lens = np.minimum(g.integers(0, 30, (n, 128)), max_new[:, None])
    full = g.random(n) < 0.5
    lens[full] = max_new[full, None]                                  # (half of the groups: every row given to the end)
    bud = g.integers(1, 30, (n, 128))
    has_bud = g.integers(0, 2, n)
    P = g.integers(1, 20, n)
    n_ctx = np.where(g.random(n) < 0.2, P + g.integers(1, 12, n), 448)
    bits = np.full(n, SERVED_BITS)
    odd = g.random(n) < 0.4
    bits[odd] = SERVED_BITS ^ (1 << g.integers(0, 14, int(odd.sum())))   # one bit flipped: a reason each
    both = g.random(n) < 0.05
    bits[both] = g.integers(0, 1 << 14, int(both.sum()))
    want = R.plan_table(G, width, lens, bud, has_bud, max_new, P, n_ctx, bits)
    got = batch(lib, G, width, lens, bud, has_bud, max_new, P, n_ctx, bits)
    assert np.array_equal(got, want)
    counts = np.bincount(want[:, 0], minlength=17)
    print("reasons:", counts.tolist())
    assert np.array_equal(np.bincount(got[:, 0], minlength=17), counts)
    assert np.all(counts > 0), counts.tolist()                        # served, and every reason of the rule
    sv = want[want[:, 0] == R.SERVED]
    assert sv[:, 1].min() == 2 and sv[:, 1].max() == 8 and sv[:, 3].max() >= 10
    # the single-case hook is the batch's
    for i in (0, 1, 2, 3):
        out = np.zeros(4, np.int32)
        l, b_ = np.ascontiguousarray(lens[i], np.int32), np.ascontiguousarray(bud[i], np.int32)
        assert lib.wmdbg_given_panel_plan(int(G[i]), int(width[i]), l.ctypes.data_as(IP), b_.ctypes.data_as(IP) if has_bud[i] else None,
                                          int(max_new[i]), int(P[i]), int(n_ctx[i]), int(bits[i]), out.ctypes.data_as(IP)) == 0
        assert out.tolist() == want[i].tolist()


def test_the_plan_by_hand():
    # 5 rows given 12 of 12: indices [1, 12) in two rounds of 8 and 3
    assert R.plan(5, 8, [12] * 5, None, 12, 4, 64, SERVED_BITS) == (R.SERVED, 8, 12, 2)
    assert R.rounds_of(8, 12) == [(1, 8), (9, 3)]
    # lengths 12 / 7 / 3 / 12 / 1 with budgets equal to them: every row is given or finished everywhere
    assert R.plan(5, 8, [12, 7, 3, 12, 1], [12, 7, 3, 12, 1], 12, 4, 64, SERVED_BITS) == (R.SERVED, 8, 12, 2)
    # ... without budgets the shortest text ends the phase: lens 1 leaves nothing
    assert R.plan(5, 8, [12, 7, 3, 12, 1], None, 12, 4, 64, SERVED_BITS)[0] == R.NO_PHASE
    assert R.plan(5, 8, [12, 7, 3, 12, 4], None, 12, 4, 64, SERVED_BITS) == (R.SERVED, 8, 3, 1)
    # a prefix of 4 with budgets 12: [1, 4)
    assert R.plan(5, 3, [4] * 5, [12] * 5, 12, 4, 64, SERVED_BITS) == (R.SERVED, 3, 4, 1)
    # a free row: no phase; 65 rows: too narrow; 64 rows: width 2
    assert R.plan(3, 8, [5, 0, 5], None, 5, 4, 64, SERVED_BITS)[0] == R.NO_PHASE
    assert R.plan(65, 8, [5] * 65, None, 5, 4, 64, SERVED_BITS)[0] == R.NARROW
    assert R.plan(64, 8, [5] * 64, None, 5, 4, 64, SERVED_BITS) == (R.SERVED, 2, 5, 2)
    # the context's end: P + L - 1 < n_text_ctx
    assert R.plan(1, 4, [9], None, 9, 4, 10, SERVED_BITS) == (R.SERVED, 4, 6, 2)


# ---------------------------------------------------------------- the round restatement
TS = (8, 5, 16)   # ts_begin, eot, n_vocab: ids 0 .. 4 text, 5 eot, 8 .. 15 timestamps


def state(G, n_ctx, P, texts, first_tok, max_new, ts=True):
    """the state behind the ordinary step at P - 1, which wrote first_tok[c] at position P"""
    from spec_ref import ts_advance, ts_start
    stride = max(len(t) for t in texts)
    st = dict(seq=[[-1] * G for _ in range(n_ctx)], lens=[len(t) for t in texts], tok=[list(t) + [0] * (stride - len(t)) for t in texts],
              done=[0] * G, logprob=[[None] * G for _ in range(max_new)], hist=[], rng=[])
    for c in range(G):
        st["seq"][P][c] = first_tok[c]
        if ts:
            h, r = ts_start(TS[0], TS[2], -1)
            h, r = ts_advance(h, first_tok[c], *TS)
            st["hist"].append(list(h)); st["rng"].append(list(r))
    return st


def run_phase(st, G, w, Lp, P, n_ctx, max_new, eot, budgets, pad, ts):
    """the rounds with a close that keeps the given token, log-prob -gi (a row behind its text: the id 3)"""
    out = []
    rounds = R.rounds_of(w, Lp)
    for k, (g0, wr) in enumerate(rounds):
        rows = R.stage_round(st, G, wr, g0, P, n_ctx, ts, pad, k == 0)
        wtok, wlp = [], []
        for c in range(G):
            for s in range(wr):
                gi = g0 + s
                tok = st["tok"][c][gi] if gi < st["lens"][c] else 3
                wtok.append(tok); wlp.append(-float(gi))
        out.append((rows, R.commit_round(st, G, wr, g0, P, max_new, wtok, wlp, eot, budgets, pad, ts, k == len(rounds) - 1)))
    return out


def column(st, P, c, n):
    return [st["seq"][P + i][c] for i in range(n)]


@pytest.mark.parametrize("at", [1, 2, 3])
def test_an_eot_at_panel_row_0_in_the_middle_and_at_the_last_row(at):
    """one round of width 3 over generated indices 1 .. 3; the text holds eot at index `at`"""
    text = [1, 2, 2, 2, 2]
    text[at] = 5
    st = state(2, 12, 3, [text, [1, 1, 1, 1, 1]], [1, 1], 5, ts=False)
    (rows, (n_live, live)), _ = run_phase(st, 2, 3, 5, 3, 12, 5, 5, None, 5, None)
    assert rows is None
    assert column(st, 3, 0, 4) == [1] + text[1:at + 1] + [5] * (3 - at)          # kept up to the eot, pads behind
    assert [st["logprob"][gi][0] for gi in (1, 2, 3)] == [-float(gi) if gi <= at else 0.0 for gi in (1, 2, 3)]
    assert st["done"] == [1, 0] and (n_live, live) == (1, [1]) and st["pos"] == 7      # (behind the second round of width 1)
    assert column(st, 3, 1, 5) == [1, 1, 1, 1, 1] and st["logprob"][4] == [0.0, -4.0]   # the second round: window 0 pads


@pytest.mark.parametrize("budget, done_after, kept", [(1, 1, 0), (3, 1, 2), (4, 1, 3), (5, 1, 4), (6, 0, 4)])
def test_a_budget_in_front_of_inside_at_and_behind_a_panel(budget, done_after, kept):
    """one round of width 4 over generated indices 1 .. 4: the budget ended at index 0 (the ordinary step set done), ends inside,
    at the panel's last row, one behind it in a second round, or not at all within max_new = 5"""
    st = state(1, 12, 2, [[1, 2, 3, 4, 1]], [1], 5, ts=False)
    if budget == 1:
        st["done"][0] = 1
    res = run_phase(st, 1, 4, 5, 2, 12, 5, -1, [budget], 0, None)
    n1 = res[0][1][0]
    want = [2, 3, 4, 1][:min(kept, 4)]
    got = column(st, 3, 0, 4)
    assert got[:len(want)] == want and got[len(want):] == [0] * (4 - len(want))
    assert st["done"][0] == done_after and n1 == (0 if budget <= 5 else 1) and st["pos"] == 6
    assert [st["logprob"][gi][0] for gi in range(1, 5)] == [-float(gi) if gi <= len(want) else 0.0 for gi in range(1, 5)]
    if budget == 5:                                                                 # (done by the last row of the round)
        assert res[0][1] == (0, [])


def test_a_frozen_window_beside_live_ones_and_a_forced_closing_timestamp():
    """three windows under the rules, rounds of width 2 over indices 1 .. 4; window 1 was finished by the ordinary step; window 2's
    text opens a timestamp at index 3 and goes on with a text id at index 4 -- row s = 1 of the second round -- where the rules
    want the closing timestamp (or eot): that row's staged ranges leave the id out (the kernel answers -inf), the window keeps
    the given id all the same and its rule state follows it"""
    texts = [[8, 1, 9, 9, 2], [8, 1, 1, 1, 1], [8, 1, 1, 9, 2]]
    st = state(3, 12, 2, texts, [8, 8, 8], 5)
    st["done"][1] = 1
    res = run_phase(st, 3, 2, 5, 2, 12, 5, 5, None, 5, TS)
    rows = res[0][0]                      # row (c, 0): the committed ranges behind <|8|>; row (c, 1): behind its input, the text id 1
    assert rows[0] == st_rng_after([8]) and rows[1] == st_rng_after([8, 1]) and rows[4] == rows[0] and rows[5] == rows[1]
    rows2 = res[1][0]
    assert rows2[0] == st_rng_after([8, 1, 9]) and rows2[1] == st_rng_after([8, 1, 9, 9])
    assert rows2[4] == st_rng_after([8, 1, 1]) and rows2[5] == st_rng_after([8, 1, 1, 9])
    text_lo, text_hi, ts_lo, ts_hi = rows2[5]
    assert text_lo == TS[1] and ts_lo == 9 and not (text_lo <= 2 < text_hi)       # an open <|9|>: its partner or eot, never the id 2
    assert column(st, 2, 0, 5) == texts[0] and column(st, 2, 1, 5) == [8, 5, 5, 5, 5] and column(st, 2, 2, 5) == texts[2]
    assert st["logprob"][4] == [-4.0, 0.0, -4.0] and st["logprob"][1] == [-1.0, 0.0, -1.0]
    assert res[0][1] == (2, [0, 2]) and res[1][1] == (2, [0, 2]) and st["done"] == [0, 1, 0] and st["pos"] == 6
    assert st["rng"][0] == st_rng_after(texts[0]) and st["rng"][2] == st_rng_after(texts[2]) and st["hist"][0][0] == 5
    assert st["rng"][1] == st_rng_after([8])                                        # the frozen window's state did not move


def st_rng_after(toks):
    from spec_ref import ts_advance, ts_start
    h, r = ts_start(TS[0], TS[2], -1)
    for t in toks:
        h, r = ts_advance(h, t, *TS)
    return list(r)


# ---------------------------------------------------------------- the binding on a stand-in library
def test_set_given_panel_and_its_refusals():
    c = given_ctx()
    seen = []
    c.lib.wm_set_given_panel = type("F", (), {"__call__": lambda self, h, n: seen.append((h.value, n)) or (0 if 1 <= n <= 8 else 1)})()
    c.lib.wm_last_error = lambda: b"set_given_panel: width outside [1, 8]"
    c.set_given_panel(4)
    c.set_given_panel(np.int64(8))
    assert seen == [(0xC0DE, 4), (0xC0DE, 8)]
    assert c.lib.wm_set_given_panel.argtypes == [ctypes.c_void_p, ctypes.c_int] and c.lib.wm_set_given_panel.restype == ctypes.c_int
    for bad in (0, 9):
        with pytest.raises(B.WhisperError) as e:
            c.set_given_panel(bad)
        assert e.value.status == 1
    assert B.MAX_TEACHER_PANEL == 8


def score_log(form, texts, prompts=P3):
    c = given_ctx()
    kw = {} if form == "absent" else dict(form=form)
    out = B.score_given(c, windows(c), None, prompts, texts, 50, length_penalty=0.5, **kw)
    return c.lib.calls, out


def test_score_given_forms():
    even = [[[5, 6], [7]], [[8], [9, 10, 11]], [[12], [13]]]
    uneven = [[[5, 6]], [[8], [9, 10, 11], [4]], [[12], [13]]]
    today, _ = score_log("absent", even)
    none, out_none = score_log(None, even)
    best, _ = score_log("best_of", even)
    rows, out_rows = score_log("rows", even)
    assert none == today and best == today                                      # form=None keeps today's choice: one best-of call
    assert today[2][0] == "wm_transcribe_windows" and today[2][1]["N"] == 2 and out_none.best is not None
    call = rows[2][1]
    assert [x[0] for x in rows] == ["wm_set_token_budgets", "wm_set_given_tokens", "wm_transcribe_windows"]
    assert call["N"] == 1 and call["B"] == 6 and call["rows"]["values"] == [0, 0, 1, 1, 2, 2]
    assert rows[0][1]["budgets"]["values"] == [3, 2, 2, 4, 2, 2] and rows[1][1]["lens"] == [3, 2, 2, 4, 2, 2]
    assert out_rows.best is None and [len(r) for r in out_rows.logprobs] == [2, 2, 2]
    # uneven counts: None and "rows" are the repeated-rows call, "best_of" does not apply
    u_today, _ = score_log("absent", uneven, RAGGED)
    u_none, _ = score_log(None, uneven, RAGGED)
    u_rows, _ = score_log("rows", uneven, RAGGED)
    assert u_none == u_today and u_rows == u_today and u_today[2][1]["N"] == 1
    with pytest.raises(ValueError, match="best_of"):
        score_log("best_of", uneven, RAGGED)
    with pytest.raises(ValueError, match="form"):
        score_log("panels", even)


def test_without_a_form_the_pinned_call_logs_are_the_parents():
    with open(BC.GOLDEN_FILE) as f:
        golden = BC.json.load(f)["cases"]
    for name in sorted(BC.CASES):
        assert BC.run_case(name) == golden[name], name
