"""CPU tests of the pure host half of speculative decoding (tx_plan.cpp: wm_spec_groups, wm_spec_width, wm_spec_round; the
per-window rules of csrc/spec_round.h, which the commit kernel of spec.hip shares) against tests/spec_ref.py: every combination
of the windows' states for G <= 4 windows x w <= 4 rows (the full product, see _window_states for what a state is), and random
cases up to 16 x 8 with all-frozen groups and a budget of 0."""
import ctypes
import itertools

import numpy as np
import pytest

import spec_ref as S

vp, ip = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_spec_groups.argtypes = [ip, ip, ip, vp, vp]
    lib.wmdbg_spec_groups.restype = ip
    lib.wmdbg_spec_width.argtypes = [ip, ip, ip]
    lib.wmdbg_spec_width.restype = ip
    lib.wmdbg_spec_round.argtypes = [ip, ip, vp, vp, vp, vp, vp, vp]
    lib.wmdbg_spec_round.restype = ip
    return lib


def _p(a):
    return a.ctypes.data_as(vp)


def _round(lib, w, acc, live, eot_at, left):
    G = len(acc)
    a, l, e, f = (np.array(x, dtype=np.int32) for x in (acc, live, eot_at, left))
    live_out = np.full(G, -7, dtype=np.int32)
    inc = np.full((G, 4), -7, dtype=np.int32)
    n = lib.wmdbg_spec_round(G, w, _p(a), _p(l), _p(e), _p(f), _p(live_out), _p(inc))
    return n, live_out.tolist(), [tuple(r) for r in inc.tolist()]


def _window_states(w):
    """Every state of one window at width w, (accepted, live, eot_at, left), up to equivalence: a frozen window's other fields
    are not read; a live one has accepted = 0 .. w - 1 leading matches, the first end-of-text among its accepted + 1 tokens at
    eot_at = -1 (none) or 0 .. accepted, and left = 1 .. accepted + 1 tokens of budget -- each a different cut of its own
    tokens -- or more than accepted + 1, where the budget plays no part in the round (spec_round.h compares left with
    accepted + 1 and with the cut n <= accepted + 1 only): accepted + 2 stands for all of them."""
    out = [(0, 0, -1, 1)]
    for a in range(w):
        for e in range(-1, a + 1):
            for left in range(1, a + 3):
                out.append((a, 1, e, left))
    return out


def _batch(lib, G, w, cases):
    n = len(cases)
    inp = np.ascontiguousarray(np.array(cases, dtype=np.int32).transpose(0, 2, 1))      # [n][G][4] -> [n][4][G]
    out = np.full((n, 1 + 5 * G), -7, dtype=np.int32)
    assert lib.wmdbg_spec_round_batch(n, G, w, _p(inp), _p(out)) == n
    return out


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_round_exhaustive(lib, G):
    """wm_spec_round for EVERY combination of the windows' states (the full product: 55 states per window at w = 4, 55 ^ 4 =
    9.2 million cases at G = 4), w = 1 .. 4.  The library's side runs in batches; the expectation is spec_ref's rules laid out
    as tables so that numpy can compare the product: what a state asks of the minimum (spec_ref.window_ask), n = the minimum
    of the live windows' asks capped at w, and a window's results as a function of its own state and n (window_own /
    window_stops) -- spec_ref.spec_round's own two steps; test_the_tables_are_spec_refs_round holds them to it case by case."""
    lib.wmdbg_spec_round_batch.argtypes = [ip, ip, ip, vp, vp]
    lib.wmdbg_spec_round_batch.restype = ip
    total = 0
    for w in (1, 2, 3, 4):
        st, ask, per = _tables(w)
        S_ = len(st)
        N = S_ ** G
        for lo in range(0, N, 1 << 20):
            flat = np.arange(lo, min(N, lo + (1 << 20)), dtype=np.int64)
            chunk = np.stack(np.unravel_index(flat, (S_,) * G), axis=1)                # every combination of states
            got = _batch(lib, G, w, st[chunk])
            live_any = st[chunk][:, :, 1].any(axis=1)
            n_want = np.where(live_any, np.minimum(ask[chunk].min(axis=1), w), 0).astype(np.int32)
            res = per[chunk, n_want[:, None]]                                          # [n][G][5]
            want = np.concatenate([n_want[:, None], res[:, :, 0], res[:, :, 1:].reshape(len(chunk), 4 * G)], axis=1)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (w, st[chunk[bad[0]]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
            total += len(chunk)
    assert total == sum(len(_window_states(w)) ** G for w in (1, 2, 3, 4))


def _tables(w):
    """(states [S][4], ask [S], per [S][w + 1][5] = (live_out, rounds, proposed, accepted, kept) of a window in that state at cut n)"""
    states = _window_states(w)
    ask = np.array([S.window_ask(a, e, l) if live else S.NO_CUT for a, live, e, l in states], dtype=np.int64)
    per = np.zeros((len(states), w + 1, 5), dtype=np.int32)
    for i, (a, live, e, l) in enumerate(states):
        for n in range(w + 1):
            if live:
                own = S.window_own(a, e, l)
                m = min(n, own)
                per[i, n] = (0 if S.window_stops(m, e, l) else 1, 1, w - 1, min(a, own), min(a, m))
    return np.array(states, dtype=np.int32), ask, per


def test_the_tables_are_spec_refs_round(lib):
    """spec_ref.spec_round itself, case by case, against the library AND the tables: every pair of states, and random groups of 3 / 4"""
    for w in (1, 2, 3, 4):
        states = _window_states(w)
        for x in states:
            for y in states:
                acc, live, eot_at, left = (list(v) for v in zip(x, y))
                want = S.spec_round(w, acc, live, eot_at, left)
                got = _round(lib, w, acc, live, eot_at, left)
                assert got == (want[0], want[1], [tuple(r) for r in want[2]]), (w, x, y)
        st, ask, per = _tables(w)
        rng = np.random.default_rng(w)
        for G in (2, 3, 4):
            for _ in range(400):
                pick = rng.integers(0, len(states), size=G)
                acc, live, eot_at, left = (list(v) for v in zip(*(states[i] for i in pick)))
                n, live_out, inc = S.spec_round(w, acc, live, eot_at, left)
                assert n == (min(int(ask[pick].min()), w) if any(live) else 0)
                assert [[lo] + list(i) for lo, i in zip(live_out, inc)] == per[pick, n].tolist()


def test_round_properties_random(lib):
    rng = np.random.default_rng(22)
    for case in range(3000):
        G = int(rng.integers(1, 17))
        w = int(rng.integers(1, 9))
        kind = case % 5
        acc = [int(v) for v in rng.integers(0, w, size=G)]
        live = [int(v) for v in rng.integers(0, 2, size=G)] if kind else [0] * G          # kind 0: an all-frozen group
        eot_at = [int(rng.integers(-1, a + 1)) if rng.integers(0, 3) == 0 else -1 for a in acc]
        left = [int(rng.integers(1, 12)) for _ in range(G)]
        if kind == 1:
            left[int(rng.integers(0, G))] = 0    # a budget of 0 is used up before any round: the window writes nothing and is done
        want = S.spec_round(w, acc, live, eot_at, left)
        got = _round(lib, w, acc, live, eot_at, left)
        assert got == (want[0], want[1], [tuple(r) for r in want[2]]), (case, w, acc, live, eot_at, left)
        n, live_out, inc = got
        assert 0 <= n <= w and (n == 0) == (not any(live))
        for c in range(G):
            if not live[c]:
                assert live_out[c] == 0 and inc[c] == (0, 0, 0, 0)
                continue
            r, p, a, k = inc[c]
            assert (r, p) == (1, w - 1) and 0 <= k <= a <= acc[c] <= p
            # a window that stays live kept exactly n tokens, none of them a stop
            if live_out[c]:
                assert n <= acc[c] + 1 and left[c] > n and not (0 <= eot_at[c] < n)


def test_group_cut(lib):
    for B in list(range(1, 40)) + [64, 127, 128, 129, 300]:
        for k in range(1, S.MAX_DRAFT_LEN + 1):
            for sg in (0, 1, 2, 3, 5, 8, 16, 64, 128, 1000):
                b0 = np.full(B, -1, dtype=np.int32)
                cg = np.full(B, -1, dtype=np.int32)
                G = lib.wmdbg_spec_groups(B, k, sg, _p(b0), _p(cg))
                wb0, wcg = S.spec_groups(B, k, sg)
                assert G == len(wb0) and b0[:G].tolist() == wb0 and cg[:G].tolist() == wcg, (B, k, sg)
                assert sum(wcg) == B and max(wcg) - min(wcg) <= 1 and max(wcg) * (k + 1) <= S.DEC_MAXB
                assert max(wcg) <= (sg if sg > 0 else S.DEFAULT_GROUP)
    assert lib.wmdbg_spec_groups(0, 3, 0, None, None) == -1 and lib.wmdbg_spec_groups(4, 8, 0, _p(b0), _p(cg)) == -1


def test_width(lib):
    for k in range(1, 8):
        for last in (3, 10, 446):
            for bound in range(0, last + 3):
                w = lib.wmdbg_spec_width(k, bound, last)
                assert w == S.spec_width(k, bound, last)
                assert w == 0 or (1 <= w <= k + 1 and bound + w - 1 <= last)


def test_walk_full_acceptance_and_none():
    """the walk itself on two scripts whose statistics are known in closed form"""
    max_new, P = 25, 3
    plain = [list(range(100, 100 + max_new))]
    for k in (1, 3, 7):
        (r, p, a, kept), = S.walk(plain, [max_new], plain, P, max_new, k, -1)
        assert r == -(-(max_new - 1) // (k + 1)) and a == p == kept
        (r, p, a, kept), = S.walk(plain, [max_new], [[0] * max_new], P, max_new, k, -1)
        assert r == max_new - 1 and a == kept == 0
