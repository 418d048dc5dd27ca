"""Kernel-level GPU tests of the constraint, compared EXACTLY with the numpy restatement of
tests/constraint_ref.py: the state kernel alone (wm_constraint_state through wmdbg_constraint_state: ban words and reached
states) and one decode position's logits launch + close under an automaton (wmdbg_decode_close_cst next to wmdbg_decode_close on
the same operands)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import constraint_ref as CR
import test_repetition_kernel_gpu as RK
from test_decode_step_kernels_gpu import SENT32, Step, P, allowed_sets, bits, check_embedding, decide, err_msg, lse64

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
N_CTX = 448
EOTS = RK.EOTS
UNWRITTEN = -16843010          # 0xfefefefe: the hook's pre-fill of state_out


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_constraint_state.argtypes = [vp, vp] + [ip] * 5 + [vp] * 5 + [ip, ctypes.c_int32] + [vp] * 4
    c.lib.wmdbg_decode_close.argtypes = [vp, ctypes.POINTER(Step)]
    c.lib.wmdbg_decode_close_cst.argtypes = [vp, ctypes.POINTER(Step)] + [vp] * 5 + [ip, ctypes.c_int32, vp]
    yield c
    c.close()


# =================================================================== the automata
@functools.lru_cache(maxsize=None)
def automaton(V, name):
    """chain  : one chain of 32 tokens (ids around word boundaries).
    wide   : 4096 one-token phrases -- the root's fan-out is 4096 (1000 at V = 1024: every text id).
    deep   : 512 eight-token phrases that share no prefix.
    digits : a two-state loop over ten ids (state 0 accepts, a digit leads to state 1 and back).
    but    : a default-edge state with three -1 exceptions, then one id.
    open   : an accepting start that allows everything and stays."""
    eot = EOTS[V]
    rng = np.random.default_rng(V + len(name))
    if name == "chain":
        return CR.from_choices([[(37 * i + 31) % eot for i in range(32)]], eot)
    if name == "wide":
        return shared_leaf_trie([[int(t)] for t in np.sort(rng.permutation(eot)[:min(4096, eot)])], eot)
    if name == "deep":
        firsts = rng.permutation(eot)[:512]
        return shared_leaf_trie([[int(f)] + [int(t) for t in rng.integers(0, eot, 7)] for f in firsts], eot)
    if name == "digits":
        d = list(range(50, 60))
        return CR.Automaton([0, 10, 20], d + d, [1] * 10 + [0] * 10, [-1, -1], [1, 0], eot)
    if name == "but":
        return CR.Automaton([0, 3, 4, 4], [31, 32, eot - 1, 7], [-1, -1, -1, 2], [1, -1, -1], [0, 0, 1], eot)
    assert name == "open"
    return CR.Automaton([0, 0], [], [], [0], [1], eot)


def shared_leaf_trie(choices, eot):
    """CR.from_choices for phrases none of which is a prefix of another, with ONE accepting leaf for all of them (state 1): 4096
    one-token phrases are 2 states, 512 eight-token phrases 2 + 512 * 7 -- inside WM_MAX_CST_STATES, where a leaf each is not."""
    kids = [{}, {}]
    for c in choices:
        s = 0
        for t in c[:-1]:
            if t not in kids[s]:
                kids[s][t] = len(kids)
                kids.append({})
            s = kids[s][t]
        assert c[-1] not in kids[s]
        kids[s][c[-1]] = 1
    beg, tok, nxt = [0], [], []
    for k in kids:
        tok += sorted(k)
        nxt += [k[t] for t in sorted(k)]
        beg.append(len(tok))
    return CR.Automaton(beg, tok, nxt, [-1] * len(kids), [0, 1] + [0] * (len(kids) - 2), eot)


def a_member(a, rng, start=0, max_len=40):
    """a random walk along allowed text ids from `start` -- every prefix of it is a mid-phrase history"""
    s, out = start, []
    for _ in range(max_len):
        ok = np.flatnonzero(CR.allowed(a, s)[:a.eot])
        if ok.size == 0:
            break
        t = int(ok[rng.integers(ok.size)])
        out.append(t)
        s = CR.delta(a, s, t)
    return out


def histories(V, name):
    """per automaton: empty, mid-phrase, at a leaf (or deep in the loop), with ids > eot and eot padding inside, one that leaves
    the language"""
    a, eot = automaton(V, name), EOTS[V]
    rng = np.random.default_rng(V + 7)
    full = a_member(a, rng, max_len=420 if name in ("digits", "open") else 40)
    mid = full[:max(1, len(full) // 2)]
    mixed = []
    for t in mid:
        mixed += [t, int(rng.integers(eot + 1, V))] if rng.integers(2) else [t]
    mixed += [eot, eot]
    bad = next(t for t in range(eot) if not CR.allowed(a, CR.fold(a, 0, mid))[t]) if name != "open" else None
    out = [[], mid, full, mixed]
    if bad is not None:
        out.append(mid + [bad, mid[0]])
    return out


def state_call(dbg, a, seq, pos, n_prompt, V, starts, ban_in):
    n_ctx, B = seq.shape
    words = CR.words_of(V)
    arrs = a.arrays()
    ban = np.zeros((B, words), np.uint32)
    st = np.zeros(B, np.int32)
    rc = dbg.lib.wmdbg_constraint_state(dbg.handle, P(np.ascontiguousarray(seq, np.int32)), B, n_ctx, pos, n_prompt, V,
                                        *[P(x) for x in arrs], a.S, a.eot, P(np.ascontiguousarray(starts, np.int32)),
                                        P(np.ascontiguousarray(ban_in, np.uint32)), P(ban), P(st))
    assert rc == 0, err_msg(dbg)
    return ban, st


def incoming(B, V, seed):
    """ban words with bits set below, at and above eot"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, (B, CR.words_of(V)), dtype=np.uint64).astype(np.uint32)
    return w & rng.integers(0, 2 ** 32, w.shape, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [1, 5, 17, 128])
def test_the_state_kernel_equals_the_restatement(dbg, B, V):
    """Every automaton x every history, one history per row (rows cycle through them, so B = 128 holds them all several times and
    B = 1 takes them in turn), every row from state 0 except each seventh, which is on -1.  ban_out and state_out EXACTLY: the
    incoming bits survive, a row on -1 keeps its words and its state pre-fill, no word above eot's changes."""
    eot, words = EOTS[V], CR.words_of(V)
    for name in ("chain", "wide", "deep", "digits", "but", "open"):
        a = automaton(V, name)
        assert CR.invalid(a, V) is None
        hs = histories(V, name)
        for base in range(0, len(hs), B):              # B = 1: one call per history; otherwise one call
            rows = [hs[(base + b) % len(hs)] for b in range(B)]
            n_prompt = 3
            k = max(len(h) for h in rows)
            seq = np.full((N_CTX, B), eot, np.int32)   # behind a row's own history: the padding of a finished row
            seq[:n_prompt] = 50                        # the prompt holds a digit: it never counts
            for b, h in enumerate(rows):
                seq[n_prompt:n_prompt + len(h), b] = h
            starts = np.array([-1 if b % 7 == 6 else 0 for b in range(B)], np.int32)
            ban_in = incoming(B, V, B + len(name))
            ban, st = state_call(dbg, a, seq, n_prompt + k - 1, n_prompt, V, starts, ban_in)
            for b, h in enumerate(rows):
                hist = seq[n_prompt:n_prompt + k, b]
                want, ws = CR.ban_words(a, int(starts[b]), hist, ban_in[b])
                assert np.array_equal(ban[b], want), (name, b)
                assert st[b] == (UNWRITTEN if ws is None else ws), (name, b, st[b], ws)
                assert np.array_equal(ban[b, (eot >> 5) + 1:], ban_in[b, (eot >> 5) + 1:])
            if name != "open" and B >= 5:
                assert (st == CR.DEAD).any()           # the history that leaves the language reached the dead state


def test_the_digit_loop_over_447_tokens_and_a_prompt_position(dbg):
    """The longest walk: 447 generated digits (n_prompt 1, position 447).  Per-row starts and permuted rows: row b of the
    permuted call is row perm[b] of the first.  A prompt position (k < 0) writes nothing at all."""
    V, B = 51865, 6
    a, eot = automaton(V, "digits"), EOTS[V]
    rng = np.random.default_rng(3)
    seq = np.full((N_CTX, B), 7, np.int32)
    seq[1:] = rng.integers(50, 60, (N_CTX - 1, B))
    seq[200, 2] = eot + 5                              # a timestamp inside row 2: the parity of its text tokens shifts
    seq[300:, 3] = eot                                 # row 3 finished at 299 generated tokens
    starts = np.array([0, 1, 0, 0, -1, 1], np.int32)
    ban_in = incoming(B, V, 1)
    ban, st = state_call(dbg, a, seq, 447, 1, V, starts, ban_in)
    for b in range(B):
        want, ws = CR.ban_words(a, int(starts[b]), seq[1:448, b], ban_in[b])
        assert np.array_equal(ban[b], want) and st[b] == (UNWRITTEN if ws is None else ws), b
    assert st.tolist() == [1, 0, 0, 1, UNWRITTEN, 0]
    perm = np.array([5, 3, 0, 4, 2, 1])
    ban2, st2 = state_call(dbg, a, seq[:, perm], 447, 1, V, starts[perm], ban_in[perm])
    assert np.array_equal(ban2, ban[perm]) and np.array_equal(st2, st[perm])
    # position 0 of a 5-token prompt: k = -4
    ban3, st3 = state_call(dbg, a, seq, 0, 5, V, starts, ban_in)
    assert np.array_equal(ban3, ban_in) and np.all(st3 == UNWRITTEN)
    # the last prompt position: k = 0, the start state's set
    ban4, st4 = state_call(dbg, a, seq, 4, 5, V, starts, ban_in)
    for b in range(B):
        want, ws = CR.ban_words(a, int(starts[b]), [], ban_in[b])
        assert np.array_equal(ban4[b], want) and st4[b] == (UNWRITTEN if ws is None else ws), b


def test_the_hook_refuses_what_the_call_refuses(dbg):
    V = 1024
    a = automaton(V, "but")
    seq, ban_in = np.zeros((16, 2), np.int32), np.zeros((2, CR.words_of(V)), np.uint32)
    out, st = np.zeros_like(ban_in), np.zeros(2, np.int32)

    def call(beg, tok, nxt, dn, acc, eot=a.eot, starts=(0, 0)):
        arrs = [np.ascontiguousarray(x, dt) for x, dt in ((beg, np.int32), (tok, np.int32), (nxt, np.int32), (dn, np.int32), (acc, np.uint8))]
        return dbg.lib.wmdbg_constraint_state(dbg.handle, P(seq), 2, 16, 3, 1, V, *[P(x) for x in arrs], len(dn), eot,
                                              P(np.ascontiguousarray(starts, np.int32)), P(ban_in), P(out), P(st))
    good = ([0, 3, 4, 4], [31, 32, 999, 7], [-1, -1, -1, 2], [1, -1, -1], [0, 0, 1])
    assert call(*good) == 0
    for bad in (([1, 3, 4, 4],) + good[1:], ([0, 3, 2, 4],) + good[1:], good[:1] + ([32, 31, 999, 7],) + good[2:],
                good[:1] + ([31, 32, 1000, 7],) + good[2:], good[:2] + ([-1, -1, -1, 3],) + good[3:], good[:3] + ([3, -1, -1],) + good[4:],
                good[:3] + ([1, -2, -1],) + good[4:], good[:2] + ([-1, -1, -1, -1],) + good[3:], good[:4] + ([0, 0, 0],)):
        assert call(*bad) == 1, bad
    assert call(*good, eot=V) == 1 and call(*good, eot=-1) == 1
    assert call(*good, starts=(0, 3)) == 1 and call(*good, starts=(-2, 0)) == 1


# =================================================================== the logits epilogue and the close
def with_automaton(dbg, a, starts):
    """RK.run_step calls dbg.lib.wmdbg_decode_close_rep(handle, step, penalty, ngram): this stand-in sends that call to
    wmdbg_decode_close_cst with the automaton behind it, so both share one set of operands."""
    keep = a.arrays() + (np.ascontiguousarray(starts, np.int32),)

    def close_cst(handle, step, p, n):
        assert (p, n) == (1.0, 0)
        return dbg.lib.wmdbg_decode_close_cst(handle, step, *[P(x) for x in keep[:5]], a.S, a.eot, P(keep[5]))
    lib = types.SimpleNamespace(wmdbg_decode_close_rep=close_cst, wmdbg_decode_close=dbg.lib.wmdbg_decode_close,
                                wm_last_error=dbg.lib.wm_last_error)
    return types.SimpleNamespace(lib=lib, handle=dbg.handle)


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [3, 17])
def test_close_under_an_automaton_equals_the_restatement(dbg, B, V):
    """wmdbg_decode_close_cst against the restatement applied to the SAME hook's constraint-off logits: the stored logits bit for
    bit (a ban does not change the stored value), the token the arg-max over the allowed ids, the log-prob its f64 log-softmax
    over the allowed set within 1e-4, the next row the embedding of that token; timestamp ranges off and on.  The histories are
    RK.step_inputs' (kinds A C A C A C A / C A C .. / eot, eot + 3 ..); the automaton: state 0 -A-> 1, 0 -C-> 2, 1 -C-> 0,
    2 -A-> 0, 1 and 2 also allow U1, state 0 accepts -- kind 0 ends in state 1 (C or U1: C), kind 1 in state 2 (A or U1: A), kind 2
    stays in state 0 (A, C or eot), and each third row is unconstrained (C).  The all-allowing automaton equals
    wmdbg_decode_close bit for bit in every output."""
    w = RK.world(V)
    seq, pos, n_prompt, bias, C, _ = RK.step_inputs(w, B)
    A, U1, eot, tsb = 20, w.eot - 1, w.eot, w.ts_begin
    a = CR.Automaton([0, 2, 4, 6], [A, C, C, U1, A, U1], [1, 2, 0, 0, 0, 0], [-1, -1, -1], [1, 0, 0], eot)
    assert CR.invalid(a, V) is None
    starts = np.array([-1 if b % 4 == 3 else 0 for b in range(B)], np.int32)
    on, every = with_automaton(dbg, a, starts), with_automaton(dbg, automaton(V, "open"), np.zeros(B, np.int32))
    ts_rng = np.array([(0, tsb, tsb + 3, V) if b % 2 == 0 else (eot, tsb, tsb + 3, V) for b in range(B)], np.int32)
    for rng in (None, ts_rng):
        kw = dict(seq=seq, pos=pos, n_prompt=n_prompt, bias=bias, rng=rng)
        off = RK.run_step(dbg, w, B, **kw)
        assert RK.same_step(off, RK.run_step(every, w, B, rep=(1.0, 0), **kw)) is None
        r = RK.run_step(on, w, B, rep=(1.0, 0), **kw)
        for b in range(B):
            banned = CR.banned_mask(a, int(starts[b]), seq[n_prompt:pos + 1, b], V)
            assert np.array_equal(bits(r.logits[b]), bits(off.logits[b])), b
            text, tsm = allowed_sets(V, [eot + 1, eot + 2], (), 0, None if rng is None else rng[b], 0, V - 1)
            text, tsm = text & ~banned, tsm & ~banned
            tok, forced, al, gap = decide(off.logits[b], text, tsm)
            assert tok is not None and r.tok[b] == tok, (b, r.tok[b], tok)
            row = off.logits[b].astype(np.float64)
            assert abs(float(r.logprob[b]) - (row[tok] - lse64(row[al]))) <= 1e-4, b
            if rng is None:
                assert tok == (C if starts[b] < 0 else (C, A, C)[b % 3]), (b, tok)
        assert r.logprob_written == B and np.all(bits(r.nospeech) == SENT32)
        assert np.array_equal(r.seq[pos + 1], r.tok) and np.array_equal(r.seq[:pos + 1], seq[:pos + 1])
        check_embedding(w, r, r.tok, pos, n_ctx=RK.STEP_CTX)
