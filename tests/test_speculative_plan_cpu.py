"""CPU tests of the pure host half of speculative decoding (tx_plan.cpp: wm_spec_groups, wm_spec_width, wm_spec_round; the
per-window rules of csrc/spec_round.h, which the commit kernel of spec.hip shares) against tests/spec_ref.py: every combination
of the windows' states for G <= 4 windows x w <= 4 rows (the full product, see _window_states for what a state is), and random
cases up to 16 x 8 with all-frozen groups and a budget of 0.  Then spec_ref's restatement of the device half, shown right before
tests/test_speculative_kernels_gpu.py compares the kernels with it: the timestamp rules' state against the oracle's
ApplyTimestampRules over every allowed history of up to 5 tokens, and adopt_ref / stage_ref / commit_ref on hand-worked cases."""
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


# ---------------------------------------------------------------- the timestamp rules' state against the oracle
TSB, TEOT, TV = 24, 20, 32                                  # a vocabulary of 32: text 0 .. 23 (eot 20), timestamps 24 .. 31
ALPHABET = (3, 7, TEOT, 24, 25, 27, TV - 1)                 # two text ids, eot, four ascending timestamps, the last at the top


def _oracle_sets(tokens, max_initial):
    """the allowed (text ids, timestamp ids) behind `tokens`: the finite set ApplyTimestampRules leaves, sum rule aside"""
    import torch
    from oracle import whisper_ref as R
    row = torch.zeros(TV, dtype=torch.float64)
    R.timestamp_filter(row, list(tokens), TSB, TEOT, max_initial, sum_rule=False)
    fin = torch.isfinite(row).tolist()
    return fin[:TSB], fin[TSB:]


def _hist_def(tokens):
    """model.h: n_sampled, last_is_ts, prev_is_ts (the start state's 1, then what last_is_ts was one token earlier), last_ts"""
    n, tss = len(tokens), [t for t in tokens if t >= TSB]
    prev = 1 if n == 0 else 0 if n == 1 else int(tokens[-2] >= TSB)
    return (n, int(n >= 1 and tokens[-1] >= TSB), prev, tss[-1] if tss else -1)


@pytest.mark.parametrize("max_initial,n_allowed", [(-1, 1067), (2, 744)])
def test_ts_advance_and_ts_start_against_the_oracle(max_initial, n_allowed):
    """Every history of length 0 .. 5 over ALPHABET that the rules allow -- the ORACLE decides: each token is in the finite set
    behind the tokens in front of it --: the ranges of spec_ref's state are exactly that finite set and the history is
    model.h's.  The counts are asserted, so that the filter cannot swallow the test (they are what the oracle's rules give:
    the same walk with spec_ref's own ranges, rule_histories, must find the same histories)."""
    total = sum(len(ALPHABET) ** n for n in range(6))
    covered, level = 0, [((), S.ts_start(TSB, TV, max_initial))]
    seen = []
    for n in range(6):
        nxt = []
        for toks, (hist, rng) in level:
            text, ts = _oracle_sets(toks, max_initial)
            assert text == [rng[0] <= i < rng[1] for i in range(TSB)], (toks, rng)
            assert ts == [rng[2] <= i < rng[3] for i in range(TSB, TV)], (toks, rng)
            assert tuple(hist) == _hist_def(toks), (toks, hist)
            covered += 1
            seen.append(toks)
            for t in ALPHABET:
                if (text[t] if t < TSB else ts[t - TSB]):
                    nxt.append((toks + (t,), S.ts_advance(hist, t, TSB, TEOT, TV)))
        level = nxt
    excluded = total - covered
    assert (covered, excluded) == (n_allowed, 19608 - n_allowed), "covered %d histories, excluded %d of %d" % (covered, excluded, total)
    ours, left_out = S.rule_histories(ALPHABET, (TSB, TEOT, TV, max_initial))
    assert [h[0] for h in ours] == seen and left_out == excluded
    # the situations the kernel tests index these histories for all occur
    kinds = {(h[1], h[2]) for _, h, _ in ours}
    assert {(0, 1), (0, 0), (1, 0), (1, 1)} <= kinds and any(h[3] == TV - 1 and r[2] == r[3] == TV for _, h, r in ours)


def test_ts_advance_on_tokens_the_rules_forbid():
    """the kernels replay PROPOSALS, which need not obey the rules: a falling timestamp lowers last_ts (the oracle reads the
    last timestamp of the sequence too), a text id behind an opening timestamp is text"""
    h, r = S.ts_replay(*S.ts_start(TSB, TV, -1), (27, 3, 25), (TSB, TEOT, TV, -1))
    assert (h, r) == ((3, 1, 0, 25), (TEOT, TSB, 25, TV))
    text, ts = _oracle_sets((27, 3, 25), -1)
    assert text == [TEOT <= i < TSB for i in range(TSB)] and ts == [i >= 25 for i in range(TSB, TV)]


# ---------------------------------------------------------------- stage_ref and commit_ref on hand-worked cases
X = -77                                                     # a cell nothing may write
RULES = (100, 90, 120, -1)                                  # ts_begin, eot, n_vocab, max_initial
AFTER_TS_TEXT = ([2, 0, 1, 100], [0, 100, 101, 120])        # the state behind <|100|> 5: text, or a timestamp above 100
START = ([0, 0, 1, -1], [0, 0, 100, 120])


def test_stage_ref_by_hand():
    # 1. two windows x 3 rows from the draft's tokens, rules on.  Window 0 behind "<|100|> 5" is offered 105 105: an opening
    # timestamp (its partner or eot, not below 105), then the closed pair (text only; the floor moves to 106).  Window 1 at the
    # start state is offered text 41 (anything, timestamps from 100), then the opening timestamp 110.
    st = dict(pos=3, script=None, tseq=[[1, 1] for _ in range(8)], dseq=[[X, X]] * 4 + [[105, 41], [105, 110], [X, X], [X, X]],
              chist=[AFTER_TS_TEXT[0], START[0]], crng=[AFTER_TS_TEXT[1], START[1]], tts_rng=[[X] * 4 for _ in range(7)])
    out = S.stage_ref(st, 2, 3, 2, 8, 6, 120, RULES)
    assert sorted(out) == ["tseq", "tts_rng"]
    assert out["tseq"] == [[1, 1]] * 4 + [[105, 41], [105, 110], [1, 1], [1, 1]]
    assert out["tts_rng"] == [[0, 100, 101, 120], [90, 100, 105, 120], [0, 100, 106, 100],
                              [0, 0, 100, 120], [0, 100, 100, 120], [90, 100, 110, 120], [X] * 4]
    # 2. a script, rules off: positions 5, 6, 7 are generated indices 3, 4, 5 of max_new = 5 -- ids -5 and 200 clamped into the
    # vocabulary of 120, index 5 is behind the script: the draft's token
    st = dict(pos=4, script=[[X, X, X, -5, 200]], tseq=[[1] for _ in range(10)], dseq=[[X]] * 7 + [[33]] + [[X]] * 2,
              chist=[[X] * 4], crng=[[X] * 4], tts_rng=[[X] * 4 for _ in range(4)])
    out = S.stage_ref(st, 1, 4, 2, 10, 5, 120, None)
    assert sorted(out) == ["tseq"] and out["tseq"] == [[1]] * 5 + [[0], [119], [33], [1], [1]]
    # 3. the end of the context: of positions 6, 7, 8 only 6 exists (n_ctx = 7) -- one proposal (eot: text), two slots
    st = dict(pos=5, script=None, tseq=[[1] for _ in range(7)], dseq=[[X]] * 6 + [[90]], chist=[AFTER_TS_TEXT[0]],
              crng=[AFTER_TS_TEXT[1]], tts_rng=[[X] * 4 for _ in range(4)])
    out = S.stage_ref(st, 1, 4, 2, 7, 20, 120, RULES)
    assert out["tseq"] == [[1]] * 6 + [[90]] and out["tts_rng"] == [[0, 100, 101, 120], [0, 100, 101, 120], [X] * 4, [X] * 4]


def _commit_state(G, w, n_ctx, max_new, pos, wtok, acc, done, **over):
    st = dict(pos=pos, wtok=wtok, wlp=[1000 + i for i in range(G * w)], acc=acc, done=done, budget=None,
              tseq=[[10 * p + c for c in range(G)] for p in range(n_ctx)], dseq=[[X] * G for _ in range(n_ctx)],
              logprob=[[X] * G for _ in range(max_new)], stats=[[5, 6, 7, 8] for _ in range(G)],
              chist=[list(START[0]) for _ in range(G)], crng=[list(START[1]) for _ in range(G)],
              dchist=[list(START[0]) for _ in range(G)], dcrng=[list(START[1]) for _ in range(G)],
              dts_hist=[[X] * 4 for _ in range(G)], dts_rng=[[X] * 4 for _ in range(G)])
    st.update(over)
    return st


def test_commit_ref_by_hand():
    # 1. 2 windows x 3 rows at pos 3 (generated index 2), rules on both sides.  Window 0 is live with one proposal accepted
    # (2 tokens of its own: <|105|> 7); window 1 is frozen.  n = 2: window 0 keeps both, window 1 pads with eot.
    st = _commit_state(2, 3, 8, 10, 3, [105, 7, 8, 55, 56, 57], [1, 2], [0, 1],
                       chist=[AFTER_TS_TEXT[0], [X] * 4], crng=[AFTER_TS_TEXT[1], [X] * 4], dchist=[AFTER_TS_TEXT[0], START[0]],
                       dcrng=[AFTER_TS_TEXT[1], START[1]])
    out = S.commit_ref(st, 2, 3, 2, 8, 10, 90, 90, RULES, RULES)
    assert out["tseq"] == [[0, 1], [10, 11], [20, 21], [30, 31], [105, 90], [7, 90], [60, 61], [70, 71]]      # row 6: a proposal, left
    assert out["dseq"] == [[X, X]] * 5 + [[7, 90]] + [[X, X]] * 2
    assert out["logprob"] == [[X, X]] * 2 + [[1000, 0], [1001, 0]] + [[X, X]] * 6
    assert out["done"] == [0, 1] and out["stats"] == [[6, 8, 8, 9], [5, 6, 7, 8]]
    # behind <|100|> 5 <|105|> 7: text, or a timestamp above 105; the frozen window's committed state is not touched
    assert out["chist"] == [[4, 0, 1, 105], [X] * 4] and out["crng"] == [[0, 100, 106, 120], [X] * 4]
    # the draft: its committed state along the group's 2 tokens -- window 1's padding (eot, text) included
    assert out["dchist"] == out["dts_hist"] == [[4, 0, 1, 105], [2, 0, 0, -1]]
    assert out["dcrng"] == out["dts_rng"] == [[0, 100, 106, 120], [0, 100, 100, 120]]
    assert (out["n_live"], out["round"], out["tpos"], out["dpos"]) == (1, [1, 5], 5, 5)
    # 2. nobody is live: nothing moves; the draft's running state is its committed one
    st = _commit_state(2, 3, 8, 10, 3, [1, 2, 3, 4, 5, 6], [2, 0], [1, 1])
    out = S.commit_ref(st, 2, 3, 2, 8, 10, 90, 90, RULES, RULES)
    for k in ("tseq", "dseq", "logprob", "done", "stats", "chist", "crng", "dchist", "dcrng"):
        assert out[k] == st[k], k
    assert out["dts_hist"] == st["dchist"] and out["dts_rng"] == st["dcrng"]
    assert (out["n_live"], out["round"], out["tpos"], out["dpos"]) == (0, [0, 3], 3, 3)
    # 3. rules off.  Window 0 has all accepted and its second token is eot: it would stop among its own tokens and asks nothing
    # of the cut; window 1 misses at row 0: n = 1.  Window 0 keeps the first of its 2 tokens and stays live.
    st = _commit_state(2, 3, 8, 10, 3, [5, 90, 6, 9, 9, 9], [2, 0], [0, 0])
    out = S.commit_ref(st, 2, 3, 2, 8, 10, 90, 90, None, None)
    assert sorted(out) == sorted(["tseq", "dseq", "logprob", "done", "stats", "n_live", "round", "tpos", "dpos"])
    assert out["tseq"][4] == [5, 9] and out["tseq"][5] == [50, 51] and out["dseq"][4] == [5, 9]
    assert out["logprob"][2] == [1000, 1003] and out["logprob"][3] == [X, X]
    assert out["done"] == [0, 0] and out["stats"] == [[6, 8, 9, 9], [6, 8, 7, 8]]    # window 0: both own tokens were proposed, 1 kept
    assert (out["n_live"], out["round"]) == (2, [2, 4])
    # 4. one window, all accepted, early stop off, max_new = 4 ends inside the panel (2 tokens left): every live window stops,
    # so the group moves the whole width; the third token is padding (id 0) and its log-prob slot does not exist
    st = _commit_state(1, 3, 8, 4, 3, [11, 12, 13], [2], [0])
    out = S.commit_ref(st, 1, 3, 2, 8, 4, -1, 0, None, None)
    assert [r[0] for r in out["tseq"]] == [0, 10, 20, 30, 11, 12, 0, 70] and out["dseq"][6] == [0]
    assert out["logprob"] == [[X], [X], [1000], [1001]] and out["done"] == [1] and out["stats"] == [[6, 8, 9, 10]]
    assert (out["n_live"], out["round"], out["tpos"]) == (0, [0, 6], 6)
    # the same with a budget of 3 instead (max_new = 10): one token left
    st = _commit_state(1, 3, 8, 10, 3, [11, 12, 13], [2], [0], budget=[3])
    out = S.commit_ref(st, 1, 3, 2, 8, 10, -1, 0, None, None)
    assert [r[0] for r in out["tseq"]][4:7] == [11, 0, 0] and out["logprob"][2:5] == [[1000], [0], [0]] and out["stats"] == [[6, 8, 8, 9]]


def test_adopt_ref_by_hand():
    st = dict(tseq=[[1, 1], [2, 2], [105, 5]], dseq=[[X, X] for _ in range(3)], stats=[[X] * 4] * 3,
              tts_hist=[[1, 1, 0, 105], [1, 0, 0, -1]], tts_rng=[[0, 100, 106, 100], [0, 100, 100, 120]])
    for k in ("chist", "crng", "dts_hist", "dts_rng", "dchist", "dcrng"):
        st[k] = [[X] * 4 for _ in range(3)]
    out = S.adopt_ref(st, 2, 2, RULES, (100, 90, 110, 3))
    assert out["dseq"] == [[X, X], [X, X], [105, 5]] and out["stats"] == [[0] * 4, [0] * 4, [X] * 4]
    assert out["chist"] == st["tts_hist"] + [[X] * 4] and out["crng"] == st["tts_rng"] + [[X] * 4]
    # the draft's own parameters (a vocabulary of 110): the first timestamp alone closes a pair; text at the start is replayed as text
    assert out["dts_hist"] == out["dchist"] == [[1, 1, 0, 105], [1, 0, 0, -1], [X] * 4]
    assert out["dts_rng"] == out["dcrng"] == [[0, 100, 106, 100], [0, 100, 100, 110], [X] * 4]
    assert sorted(S.adopt_ref(st, 2, 2, None, None)) == ["dseq", "stats"]
