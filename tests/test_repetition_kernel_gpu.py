"""Kernel-level GPU tests of the repetition rules, compared EXACTLY with the numpy restatement of
tests/repeat_ref.py: the state kernel alone (wm_repeat_state through wmdbg_repeat_state) and one decode position's logits
launch + close with the rules on (DE_LOGITS_XR through wmdbg_decode_close_rep, next to wmdbg_decode_close on the same
operands)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import repeat_ref as RR
from test_decode_step_kernels_gpu import SENT32, Step, P, allowed_sets, bf, bits, check_embedding, decide, err_msg, lse64
from test_transcribe_options_cpu import gumbel_np

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
N_CTX = 448
NGRAMS = [1, 2, 3, 8, 32]
EOTS = {1024: 1000, 51865: 50257}


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_repeat_state.argtypes = [vp, vp] + [ip] * 7 + [vp, vp]
    c.lib.wmdbg_decode_close.argtypes = [vp, ctypes.POINTER(Step)]
    c.lib.wmdbg_decode_close_rep.argtypes = [vp, ctypes.POINTER(Step), ctypes.c_float, ip]
    yield c
    c.close()


# =================================================================== A. the state kernel
@functools.lru_cache(maxsize=None)
def history_pool(V, eot):
    """16 histories of 447 tokens (a call reads a prefix): random, few ids (0, 31, 32, eot - 1: both sides of a word boundary),
    all equal, period 2 with V - 1, ids >= eot inside the repeated suffix and as the would-be banned id, heavy repeats."""
    rng = np.random.default_rng(V)
    L = N_CTX - 1
    few = np.array([0, 31, 32, eot - 1])
    rows = [rng.integers(0, V, L), few[rng.integers(0, 4, L)], np.full(L, 32), np.tile([31, V - 1], L)[:L],
            np.tile([5, eot, 9], L)[:L], np.tile([7, eot + 1], L)[:L], rng.integers(0, 6, L), rng.integers(eot - 3, eot + 3, L),
            np.tile([0, 31, 32, V - 1, 63, 64], L)[:L], rng.integers(V - 40, V, L), np.full(L, V - 1), np.full(L, 0),
            np.tile(rng.integers(0, V, 33), L)[:L], np.tile(rng.integers(0, V, 32), L)[:L], rng.integers(0, 2, L),
            np.tile([1, 2, 3, 1, 2, 4], L)[:L]]
    return np.stack(rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def want_words(V, eot, h, k, n):
    g = history_pool(V, eot)[h, :k]
    return RR.bitmap(RR.seen_set(g, eot), V), RR.bitmap(RR.ban_set(g, n, eot), V)


def state_call(dbg, seq, pos, n_prompt, V, n, eot):
    n_ctx, B = seq.shape
    words = RR.words_of(V)
    seen, ban = np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32)
    rc = dbg.lib.wmdbg_repeat_state(dbg.handle, P(np.ascontiguousarray(seq, np.int32)), B, n_ctx, pos, n_prompt, V, n, eot, P(seen), P(ban))
    assert rc == 0, err_msg(dbg)
    return seen, ban


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [1, 5, 16, 17, 128])
def test_state_kernel_rebuilds_both_bitmaps(dbg, B, V):
    """Every word of both bitmaps, exactly, for n in {1, 2, 3, 8, 32} at k in {447, n, n - 1, n - 2, 0} generated tokens -- in
    that order on ONE context, so every call after the first has a shorter history than the one before it (a stale bit would
    show; the hook pre-fills the outputs with 0xff, so an unwritten word shows too) --, then the longest one again with the
    rows permuted.  The prompt rows hold ids that would set bits if they were read."""
    eot = EOTS[V]
    pool = history_pool(V, eot)
    n_prompt = 1
    hs = [(b * 5 + B) % 16 for b in range(B)]           # row b's history (rows above 16 repeat them in another order)
    seq = np.empty((N_CTX, B), np.int32)
    seq[0] = 33                                         # the prompt: never counted
    seq[1:] = pool[hs].T
    for n in NGRAMS if B in (5, 17) else [3, 32, 1]:
        for k in (447, n, n - 1, max(n - 2, 0), 0):
            seen, ban = state_call(dbg, seq, n_prompt + k - 1 if k else 0, n_prompt if k else 1, V, n, eot)
            for b in range(B):
                ws, wb = want_words(V, eot, hs[b], k, n)
                assert np.array_equal(seen[b], ws), (n, k, b, hs[b])
                assert np.array_equal(ban[b], wb), (n, k, b, hs[b])
            if k == 0:
                assert not seen.any() and not ban.any()
    perm = np.random.default_rng(B).permutation(B)
    seen, ban = state_call(dbg, seq[:, perm], N_CTX - 1, n_prompt, V, 3, eot)
    for i, b in enumerate(perm):
        ws, wb = want_words(V, eot, hs[b], 447, 3)
        assert np.array_equal(seen[i], ws) and np.array_equal(ban[i], wb), (i, b)


def test_state_kernel_prompt_eot_and_off(dbg):
    """A longer prompt (the history starts behind it), a prompt position (pos + 1 < n_prompt: nothing), eot = V (every id is
    eligible, V - 1 included: the last, partly valid word), eot = 0 (nothing is), n = 0 (no ban, the seen bits stay)."""
    V, B = 51865, 5
    pool = history_pool(V, EOTS[V])
    seq = np.ascontiguousarray(pool[[0, 3, 9, 10, 12], :200].T)          # [200][5]
    for n_prompt, pos, n, eot in ((7, 150, 3, 50257), (7, 3, 3, 50257), (7, 6, 1, 50257), (1, 199, 2, V), (1, 199, 2, 0), (3, 120, 0, 50257),
                                  (200, 199, 2, V)):
        seen, ban = state_call(dbg, seq, pos, n_prompt, V, n, eot)
        for b in range(B):
            g = seq[n_prompt:pos + 1, b]
            assert np.array_equal(seen[b], RR.bitmap(RR.seen_set(g, eot), V)), (n_prompt, pos, n, eot, b)
            assert np.array_equal(ban[b], RR.bitmap(RR.ban_set(g, n, eot), V)), (n_prompt, pos, n, eot, b)
    seen, _ = state_call(dbg, seq, 199, 1, V, 2, V)
    assert seen[3, RR.words_of(V) - 1] == np.uint32(1) << np.uint32((V - 1) & 31)      # row 3: all V - 1


# =================================================================== B. the logits epilogue and the close
@functools.lru_cache(maxsize=None)
def world(V):
    """Operands of one vocabulary (never modified): 17 residual rows, the final LayerNorm, embeddings (K = 64)."""
    K = 64
    rng = np.random.default_rng(V + 1)
    w = types.SimpleNamespace(V=V, K=K, eot=EOTS[V], ts_begin=EOTS[V] + 10)
    w.x = (rng.standard_normal((17, K)) * (0.5 + np.arange(17) / 17)[:, None] + 0.7).astype(np.float32)
    w.g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    w.beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    w.emb = bf(rng.standard_normal((V, K)) * (2.0 / np.sqrt(K)))
    w.pemb = (rng.standard_normal((16, K)) * 0.3 + 1.0).astype(np.float32)
    return w


STEP_CTX = 16


def run_step(dbg, w, B, *, seq, pos, n_prompt, bias, rep=None, T=0.0, seed=0, chunk0=0, rng=None):
    """One wmdbg_decode_close (rep None) or wmdbg_decode_close_rep (rep = (penalty, ngram)) call in X mode on rows 0 .. B - 1."""
    V, K = w.V, w.K
    r = types.SimpleNamespace(B=B)
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a
    s = Step()
    s.B, s.V, s.K, s.n_ctx, s.pos, s.n_prompt = B, V, K, STEP_CTX, pos, n_prompt
    s.x, s.ln_g, s.ln_b, s.emb = P(arr(w.x[:B], np.float32)), P(w.g), P(w.beta), P(w.emb)
    s.bias, s.pemb = P(arr(bias, np.float32)), P(w.pemb)
    r.seq = arr(seq, np.int32).copy()
    s.seq = P(r.seq)
    sup = arr([w.eot + 1, w.eot + 2], np.int32)
    s.suppress, s.n_suppress = P(sup), sup.size
    s.arg_first, s.arg_last, s.fallback_tok = 0, V - 1, w.eot
    s.eot = w.eot                                     # the repetition rules' eot, with the timestamp rules on or off
    r.rng = r.hist = None
    if rng is not None:
        s.ts_mode, s.ts_begin, s.max_initial = 2, w.ts_begin, -1
        r.rng, r.hist = arr(rng, np.int32).copy(), arr(np.tile([3, 0, 0, -1], (B, 1)), np.int32).copy()
        s.rng, s.hist = P(r.rng), P(r.hist)
    s.x_on, s.chunk0, s.sot_pos, s.ns_tok, s.temperature, s.seed = 1, chunk0, -1, 0, T, seed
    r.logits = np.zeros((B, V), np.float32)
    r.tok, r.result = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    r.logprob, r.nospeech = np.zeros(B, np.float32), np.zeros(B, np.float32)
    r.x_next, r.xb_next, r.stats = np.zeros((B, K), np.float32), np.zeros((B, K), np.float32), np.zeros((B, 2), np.float32)
    s.logits, s.tok, s.result, s.logprob, s.nospeech = P(r.logits), P(r.tok), P(r.result), P(r.logprob), P(r.nospeech)
    s.x_next, s.xb_next, s.stats_next = P(r.x_next), P(r.xb_next), P(r.stats)
    if rep is None:
        rc = dbg.lib.wmdbg_decode_close(dbg.handle, ctypes.byref(s))
    else:
        rc = dbg.lib.wmdbg_decode_close_rep(dbg.handle, ctypes.byref(s), rep[0], rep[1])
    assert rc == 0, err_msg(dbg)
    r.logprob_written, r.pos_out, r.arrive_out, r.tail = s.logprob_written, s.pos_out, s.arrive_out, s.stats_tail_nonzero
    assert r.pos_out == pos + 1 and r.arrive_out == 0
    return r


def same_step(a, b):
    for name in ("logits", "tok", "result", "logprob", "nospeech", "x_next", "xb_next", "stats", "seq", "rng", "hist"):
        u, v = getattr(a, name), getattr(b, name)
        if u is not None and not np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)):
            return name
    return None if (a.logprob_written, a.tail) == (b.logprob_written, b.tail) else "counts"


def step_inputs(w, B):
    """Histories and a bias (shared by the rows) that make BOTH rules decide.  The bias puts C on top (130: the plain decode
    takes it in every row), A second (114), and two ids no row has generated below them, U0 (72) > U1 (50); the logits
    themselves are N(0, 2^2).  Row b's 7 generated tokens, by b % 3:
      0: A C A C A C A -- n = 2 and n = 3 ban C (the suffixes (A) and (C, A) were followed by C); A and C are seen;
      1: C A C A C A C -- the same with the roles swapped: A is banned;
      2: eot, eot + 3 alternating -- ids >= eot: nothing is seen, nothing banned.
    So under the ban alone kind 0 takes A and kind 1 keeps C; penalty 3 sends both to U0 (130 / 3 < 72), penalty 1.25 does not
    (114 / 1.25 > 72); penalty 0.5 with n = 1 doubles the seen ids and bans them: U0; kind 2 takes C whatever the rules."""
    A, C, U0, U1 = 20, 40, 27, w.eot - 1
    n_prompt, pos = 2, 8                                # k = 7 generated tokens at positions 2 .. 8
    seq = np.full((STEP_CTX, B), 33, np.int32)
    for b in range(B):
        x, y = ((A, C), (C, A), (w.eot, w.eot + 3))[b % 3]
        seq[n_prompt:pos + 1, b] = [x, y, x, y, x, y, x]
    seq[:n_prompt] = [[A], [U0]]                        # the prompt holds A and U0: it must not count
    bias = np.zeros(w.V, np.float32)
    bias[A], bias[C], bias[U0], bias[U1] = 114.0, 130.0, 72.0, 50.0
    want = {(1.0, 2): (A, C, C), (3.0, 0): (U0, U0, C), (3.0, 2): (U0, U0, C), (1.25, 3): (A, C, C), (0.5, 1): (U0, U0, C)}
    return seq, pos, n_prompt, bias, C, want


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [3, 17])
def test_close_under_the_rules_equals_the_restatement(dbg, B, V):
    """wmdbg_decode_close_rep against the restatement on the SAME hook's rules-off logits: the stored logits are the f32 penalty
    of those (bit for bit), the token is the restatement's choice on the penalised values with the banned ids out of the allowed
    sets (at T = 0.7: arg-max of value * (1 / T) + Gumbel noise; the noise is known to 1e-5 relative, so a row whose two best
    scores lie within 1e-3 may take either -- at most one row of the test), the log-prob its f64 log-softmax over the allowed
    set within 1e-4 (test_decode_step_kernels_gpu's bounds), the next row the embedding of that token.  Timestamp rules off
    and on (rows alternate: both sides admissible / text from eot only).  At the first generated token the history is
    empty: every output equals the rules-off close.  (1.0, 0) equals wmdbg_decode_close bit for bit everywhere."""
    w = world(V)
    seq, pos, n_prompt, bias, C, want = step_inputs(w, B)
    tsb, eot = w.ts_begin, w.eot
    ts_rng = np.array([(0, tsb, tsb + 3, V) if b % 2 == 0 else (eot, tsb, tsb + 3, V) for b in range(B)], np.int32)
    near = 0
    for rng in (None, ts_rng):
        for T, seed, chunk0 in ((0.0, 0, 0), (0.7, 2 ** 40 + 7, 5)):
            kw = dict(seq=seq, pos=pos, n_prompt=n_prompt, bias=bias, T=T, seed=seed, chunk0=chunk0, rng=rng)
            off = run_step(dbg, w, B, **kw)
            assert same_step(off, run_step(dbg, w, B, rep=(1.0, 0), **kw)) is None
            first = dict(kw, pos=n_prompt - 1)
            assert same_step(run_step(dbg, w, B, **first), run_step(dbg, w, B, rep=(1.5, 2), **first)) is None
            if T == 0.0 and rng is None:
                assert np.all(off.tok == C)                               # the plain decode would go on looping
            for p, n in ((1.0, 2), (3.0, 0), (3.0, 2), (1.25, 3), (0.5, 1)):
                r = run_step(dbg, w, B, rep=(p, n), **kw)
                gi = pos + 1 - n_prompt
                for b in range(B):
                    g = seq[n_prompt:pos + 1, b]
                    row32, banned = RR.apply_rules(off.logits[b], g, p, n, eot)
                    assert np.array_equal(bits(r.logits[b]), bits(row32)), (p, n, b)
                    text, tsm = allowed_sets(V, [eot + 1, eot + 2], (), 0, None if rng is None else rng[b], 0, V - 1)
                    text, tsm = text & ~banned, tsm & ~banned
                    row = row32.astype(np.float64)
                    sc = None
                    if T > 0:
                        sc = row * float(np.float32(1.0 / T)) + gumbel_np(seed, chunk0 + b, gi, np.arange(V))
                    tok, forced, al, gap = decide(row32, text, tsm, score=sc)
                    assert tok is not None
                    if T > 0 and r.tok[b] != tok:
                        best2 = np.sort(sc[al])[-2:]
                        assert best2[1] - best2[0] <= 1e-3 and al[r.tok[b]] and sc[r.tok[b]] >= best2[0] - 1e-12, (p, n, b)
                        near += 1
                        tok = int(r.tok[b])
                    assert r.tok[b] == tok, (V, B, rng is not None, T, p, n, b, r.tok[b], tok)
                    assert abs(float(r.logprob[b]) - (row[tok] - lse64(row[al]))) <= 1e-4, (p, n, b)
                    if T == 0.0 and rng is None:                          # the rules decide, as step_inputs says
                        assert tok == want[(p, n)][b % 3], (p, n, b, tok)
                assert r.logprob_written == B and np.all(bits(r.nospeech) == SENT32)
                assert np.array_equal(r.seq[pos + 1], r.tok) and np.array_equal(r.seq[:pos + 1], seq[:pos + 1])
                check_embedding(w, r, r.tok, pos, n_ctx=STEP_CTX)
    assert near <= 1, near
