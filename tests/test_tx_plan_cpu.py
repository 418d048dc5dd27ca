"""CPU test of the host arithmetic of a transcribe call (csrc/tx_plan.cpp) through the host-only hooks wmdbg_tx_plan,
wmdbg_group_tables and wmdbg_group_rows_out, against the restatement in tests/tx_plan_ref.py: the lane plan exhaustively over
call sizes, candidates, lane limits, the context's flags, model widths and the three knobs it reads; a group's tables and a
finished group's output rows over seeded random cases that cover ragged and uniform prompts, candidates, budgets above and
below max_new, and an eot nowhere, first and last.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import tx_plan_ref as ref

IP = ctypes.POINTER(ctypes.c_int32)
MAX_BEST_OF = 8   # WM_MAX_BEST_OF
PLAN_IN, PLAN_OUT, TAB_IN, TAB_OUT, ROWS_IN, ROWS_OUT = 12, 8, 256, 576, 320, 288
FILL = -77        # what the row-output buffers hold before the hook runs


@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_tx_plan.argtypes = [IP, ctypes.c_int, IP, IP, ctypes.c_int]
    for f in (lib.wmdbg_group_tables, lib.wmdbg_group_rows_out):
        f.argtypes = [IP, ctypes.c_int, IP]
    for f in (lib.wmdbg_tx_plan, lib.wmdbg_group_tables, lib.wmdbg_group_rows_out):
        f.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(IP)


# ---------------------------------------------------------------- the lane plan
B_ALL = np.arange(1, 601)
NS = (1, 2, 3, 5, 8, MAX_BEST_OF)
LANES = (1, 2, 3, 4, 8)
WIDTHS = (384, 512, 768, 1280)
KNOB_PARTS, KNOB_SOLO, KNOB_CHUNKS = (0, 1, 2, 3), (0, 8), (0, 4, 16)


def test_lane_plan_exhaustive(dbg):
    """every (B, N, lanes, explicit, prof_on, no_cu_masks, width, lane_parts, lane_solo_cus, group_chunks): L, parts, G, n_lanes,
    the kind of lane and the whole cut"""
    inner = np.array(np.meshgrid(B_ALL, (0, 1), WIDTHS, KNOB_PARTS, KNOB_SOLO, KNOB_CHUNKS, indexing="ij")).reshape(6, -1)
    n = inner.shape[1]
    B = inner[0]
    # the restatement's cut of every (B, G) once; a case's expected cut is gathered from it
    GMAX = 64
    pairs_B, pairs_G = [x.reshape(-1) for x in np.meshgrid(B_ALL, np.arange(1, GMAX), indexing="ij")]
    tab, tab_start = ref.balanced_cuts(pairs_B, pairs_G)
    tab = tab.astype(np.int32)
    done = 0
    for N, lanes, explicit, prof in itertools.product(sorted(set(NS)), LANES, (0, 1), (0, 1)):
        L, parts, G, n_lanes, kind = ref.plan(B, N, lanes, explicit, prof, *inner[1:])
        assert G.max() < GMAX
        start = np.cumsum(2 * G) - 2 * G
        total = int(2 * G.sum())
        cut_want = tab[np.repeat(tab_start[(B - 1) * (GMAX - 1) + G - 1] - start, 2 * G) + np.arange(total)]
        a = np.zeros((n, PLAN_IN), dtype=np.int32)
        a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4] = B, N, lanes, explicit, prof
        a[:, 5:10] = inner[1:].T
        out = np.full((n, PLAN_OUT), -1, dtype=np.int32)
        cut = np.full(total + 8, -1, dtype=np.int32)
        assert dbg.wmdbg_tx_plan(_p(a), n, _p(out), _p(cut), len(cut)) == n
        what = "N=%d lanes=%d explicit=%d prof_on=%d" % (N, lanes, explicit, prof)
        for i, (name, want) in enumerate((("L", L), ("parts", parts), ("G", G), ("n_lanes", n_lanes), ("kind", kind), ("cut offset", start))):
            bad = np.nonzero(out[:, i] != want)[0]
            assert bad.size == 0, "%s: %s differs in %d of %d cases, first at input %s: plan %d, restatement %d" % (
                what, name, bad.size, n, a[bad[0], :10].tolist(), out[bad[0], i], want[bad[0]])
        assert not out[:, 6:].any()
        bad = np.nonzero(cut[:total] != cut_want)[0]
        assert bad.size == 0, "%s: the cut differs at entry %d (%d entries differ)" % (what, bad[0], bad.size)
        assert (cut[total:] == -1).all()
        # what the scheduler relies on: no group is empty or above the row cap, no lane is without a group
        assert (G >= 1).all() and (G <= B).all() and (-(-B // G) * N <= ref.DEC_MAXB).all()
        assert (n_lanes >= 1).all() and (n_lanes <= G).all()
        done += n
    assert done == 600 * 5 * 5 * 2 * 2 * 2 * 4 * 4 * 2 * 3   # (N: WM_MAX_BEST_OF is 8, listed twice)


def test_lane_plan_refuses_what_it_cannot_cut(dbg):
    out = np.zeros(PLAN_OUT, dtype=np.int32)
    cut = np.zeros(16, dtype=np.int32)
    ok = np.array([40, 1, 3, 0, 0, 0, 384, 0, 0, 0, 0, 0], dtype=np.int32)
    assert dbg.wmdbg_tx_plan(_p(ok), 1, _p(out), _p(cut), 16) == 1 and out[:5].tolist() == [3, 2, 2, 2, ref.PARTS]
    assert cut[:4].tolist() == [0, 20, 20, 20]
    assert dbg.wmdbg_tx_plan(_p(ok), 1, _p(out), _p(cut), 3) == -1          # no room for the cut
    for i, v in ((0, 0), (1, 0), (1, 129), (2, 0), (9, -1)):
        bad = ok.copy()
        bad[i] = v
        assert dbg.wmdbg_tx_plan(_p(bad), 1, _p(out), _p(cut), 16) == -1


# ---------------------------------------------------------------- a group's tables
def _table_cases(rng, n):
    """n random groups of random calls: (hook input row, the restatement's arguments)"""
    rows, args = [], []
    while len(rows) < n:
        N = int(rng.integers(1, 5))
        Cg = int(rng.integers(1, 12 // N + 1))
        B = int(rng.integers(Cg, 17))
        b0 = int(rng.integers(0, B - Cg + 1))
        ragged = bool(rng.integers(0, 2))
        stride = int(rng.integers(1, 10)) if ragged or rng.integers(0, 3) else 0
        n_prompt = int(rng.integers(1, stride + 1)) if stride else int(rng.integers(1, 10))
        plen = rng.integers(1, stride + 1, size=B) if ragged else None
        budgets = rng.integers(1, 12, size=B) if rng.integers(0, 2) else None
        ids = rng.integers(0, 2 ** 31 - 1, size=B) if rng.integers(0, 2) else None
        want_ids = int(rng.integers(0, 4) > 0)
        prompts = rng.integers(0, 51864, size=max(B * stride, n_prompt))
        r = np.zeros(TAB_IN, dtype=np.int32)
        r[:10] = [B, b0, Cg, N, stride, ragged, n_prompt, budgets is not None, ids is not None, want_ids]
        if ragged:
            r[16:16 + B] = plen
        if budgets is not None:
            r[32:32 + B] = budgets
        if ids is not None:
            r[48:48 + B] = ids
        r[64:64 + len(prompts)] = prompts
        rows.append(r)
        args.append((prompts, stride, plen, n_prompt, budgets, ids, b0, Cg, N, bool(want_ids)))
    return np.stack(rows), args


def test_group_tables(dbg):
    rng = np.random.default_rng(20)
    a, args = _table_cases(rng, 3000)
    out = np.full((len(a), TAB_OUT), -1, dtype=np.int32)
    assert dbg.wmdbg_group_tables(_p(a), len(a), _p(out)) == len(a)
    seen = set()
    for i, arg in enumerate(args):
        P, table, off, bud, ids = ref.group_tables(*arg)
        what = "case %d %s" % (i, a[i, :10].tolist())
        want = [P, table.size, 0 if off is None else off.size, 0 if bud is None else bud.size, 0 if ids is None else ids.size]
        assert out[i, :5].tolist() == want, what
        assert not out[i, 5:16].any(), what
        for at, v, room in ((16, table.reshape(-1), 192), (208, off, 16), (224, bud, 16), (240, ids, 336)):
            k = 0 if v is None else v.size
            assert k == 0 or np.array_equal(out[i, at:at + k], v), what
            assert not out[i, at + k:at + room].any(), what
        seen.add((arg[2] is not None, arg[8] > 1, arg[4] is not None, arg[5] is not None, arg[9], arg[1] == 0))
    # ragged x candidates x budgets x sample ids x extended decode all met, and the one-prompt-for-all form
    assert len({s[:5] for s in seen}) == 32 and any(s[5] for s in seen)


def test_group_tables_refuses_rows_outside_the_call(dbg):
    a, _ = _table_cases(np.random.default_rng(3), 1)
    out = np.zeros((1, TAB_OUT), dtype=np.int32)
    assert dbg.wmdbg_group_tables(_p(a), 1, _p(out)) == 1
    a[0, 1] = a[0, 0]   # b0 = B
    assert dbg.wmdbg_group_tables(_p(a), 1, _p(out)) == -1


# ---------------------------------------------------------------- a group's output rows
EOT = 9


def _row_cases(rng, n):
    rows, args = [], []
    while len(rows) < n:
        N = int(rng.integers(1, 5))
        Cg = int(rng.integers(1, 12 // N + 1))
        Bg = Cg * N
        B = int(rng.integers(Cg, 16 // N + 1))
        b0 = int(rng.integers(0, B - Cg + 1))
        max_new = int(rng.integers(1, 8))
        eot = EOT if rng.integers(0, 4) else -1
        gen = rng.integers(0, 9, size=(max_new, Bg))          # no eot anywhere ...
        for b in range(Bg):                                     # ... then at position 0, at the last position, somewhere, nowhere
            how = int(rng.integers(0, 5))
            if how == 0:
                gen[0, b] = EOT
            elif how == 1:
                gen[max_new - 1, b] = EOT
            elif how == 2:
                gen[rng.integers(0, max_new):, b] = EOT
        budgets = rng.integers(1, max_new + 3, size=B) if rng.integers(0, 2) else None   # below, at and above max_new
        lp = rng.standard_normal((max_new, Bg)).astype(np.float32)
        ns = rng.random(Bg).astype(np.float32)
        want_lp, want_ns = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        r = np.zeros(ROWS_IN, dtype=np.int32)
        r[:9] = [B, b0, Bg, N, max_new, eot, budgets is not None, want_lp, want_ns]
        r[16:16 + gen.size] = gen.reshape(-1)
        r[144:144 + lp.size] = lp.reshape(-1).view(np.int32)
        r[272:272 + Bg] = ns.view(np.int32)
        if budgets is not None:
            r[288:288 + B] = budgets
        rows.append(r)
        args.append((gen, lp, ns, budgets, eot, N, b0, Bg, max_new, B, want_lp, want_ns))
    return np.stack(rows), args


def test_group_rows_out(dbg):
    rng = np.random.default_rng(21)
    a, args = _row_cases(rng, 3000)
    out = np.full((len(a), ROWS_OUT), FILL, dtype=np.int32)
    assert dbg.wmdbg_group_rows_out(_p(a), len(a), _p(out)) == len(a)
    seen = set()
    for i, (gen, lp, ns, budgets, eot, N, b0, Bg, max_new, B, want_lp, want_ns) in enumerate(args):
        tokens = np.full((16, max_new), FILL, dtype=np.int32)
        lens = np.full(16, FILL, dtype=np.int32)
        logprobs = np.full((16, max_new), FILL, dtype=np.int32).view(np.float32)
        no_speech = np.full(16, FILL, dtype=np.int32).view(np.float32)
        ref.group_rows_out(gen, lp, ns, budgets, eot, N, b0, Bg, max_new, tokens, lens, logprobs if want_lp else None,
                           no_speech if want_ns else None)
        what = "case %d %s" % (i, a[i, :9].tolist())
        R = B * N
        assert np.array_equal(out[i, :R * max_new], tokens[:R].reshape(-1)), what
        assert np.array_equal(out[i, 128:144], lens), what
        assert np.array_equal(out[i, 144:144 + R * max_new], logprobs[:R].reshape(-1).view(np.int32)), what
        assert np.array_equal(out[i, 272:288], no_speech.view(np.int32)), what
        assert (out[i, R * max_new:128] == FILL).all() and (out[i, 144 + R * max_new:272] == FILL).all(), what
        rows = lens[b0 * N:b0 * N + Bg]
        assert (rows >= 1).all() and (rows <= max_new).all(), what
        stopped = rows < max_new
        seen.update([("eot", eot >= 0), ("budgets", budgets is not None), ("short", bool(stopped.any())),
                     ("first", bool((rows == 1).any())), ("lp", want_lp), ("ns", want_ns), ("cand", N > 1)])
    assert len(seen) == 14
