"""Kernel-level GPU tests of the sequence bias, compared EXACTLY with the numpy restatement of
tests/seqbias_ref.py: the state kernel alone (wm_seqbias_state behind wm_repeat_state, through wmdbg_seqbias_state) and one
decode position's logits launch + close with a table (DE_LOGITS_XB through wmdbg_decode_close_sb, next to wmdbg_decode_close
and wmdbg_decode_close_rep on the same operands)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import repeat_ref as RR
import seqbias_ref as SB
import test_repetition_kernel_gpu as RK
from test_decode_step_kernels_gpu import SENT32, Step, P, allowed_sets, bits, check_embedding, decide, err_msg, lse64
from test_transcribe_options_cpu import gumbel_np

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
N_CTX, CAP = 448, SB.MAX_ENTRIES
EOTS = RK.EOTS
INF = np.inf


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_seqbias_state.argtypes = [vp, vp] + [ip] * 5 + [vp] * 4 + [ip, ctypes.c_int32] + [vp] * 6
    c.lib.wmdbg_decode_close.argtypes = [vp, ctypes.POINTER(Step)]
    c.lib.wmdbg_decode_close_rep.argtypes = [vp, ctypes.POINTER(Step), ctypes.c_float, ip]
    c.lib.wmdbg_decode_close_sb.argtypes = [vp, ctypes.POINTER(Step), ctypes.c_float, ip] + [vp] * 4 + [ip]
    yield c
    c.close()


# =================================================================== A. the state kernel
def tail(V):
    """the 31 newest tokens of the `hot` history, oldest first: ids on both sides of a word boundary, one >= eot"""
    eot = EOTS[V]
    t = [(7 * i + 3) % eot for i in range(31)]
    t[5], t[20], t[30] = eot + 1, 31, 32
    return t


@functools.lru_cache(maxsize=None)
def history_pool(V):
    """8 histories of 447 tokens (a call reads a prefix).  0: `hot`, every prefix of length >= 31 ends in tail(V) -- it is
    periodic with period 31 --, so the deep table below matches it with EVERY entry; 1: the same with the newest token of each
    period changed: only the context-free entries match; 2 / 3: random; 4: few ids; 5: hot shifted by one (the contexts match
    one token late: nothing longer than the shared part); 6: all V - 1; 7: ids around eot."""
    eot, L = EOTS[V], N_CTX - 1
    rng = np.random.default_rng(V + 3)
    hot = np.tile(tail(V), L // 31 + 2)
    cold = hot.copy()
    cold[30::31] = 33
    rows = [hot[:L], cold[:L], rng.integers(0, V, L), rng.integers(0, V, L), np.array([0, 31, 32, eot - 1])[rng.integers(0, 4, L)],
            hot[1:L + 1], np.full(L, V - 1), rng.integers(eot - 3, eot + 3, L)]
    return np.stack(rows).astype(np.int32)


def hist(V, h, k):
    """the k generated tokens of pool row h that END where the pool row's period ends, so that `hot` keeps its tail for every k
    >= 31 (the rows are cut from the front: position i of the call holds pool[h, 434 - k + i])"""
    return history_pool(V)[h, 434 - k:434] if h in (0, 1) else history_pool(V)[h, :k]


@functools.lru_cache(maxsize=None)
def table(V, name):
    """(sequences, biases) of the named table.
    one  : a single 2-token entry (the hot tail's last pair).
    seven: lengths 1, 2, 2, 3, 32, 32, 2 -- two entries on one last token, a ban, an id >= eot inside, no match for a random row
           except the single token.
    ctx7 : seven entries of lengths 2 .. 32, none of length 1: a random history matches NOTHING.
    deep : 4096 = 32 context lengths (0 .. 31 newest tokens of the hot tail) x 128 last tokens: the hot row matches EVERY entry
           (32 per id, summed in table order), every other row the 128 context-free ones at least.
    wide : as many distinct last tokens as fit (4096 at 51 865 ids; 1000 x 4 at 1024): the list spans every flag word."""
    eot = EOTS[V]
    t = tail(V)
    rng = np.random.default_rng(V + len(name))
    if name == "one":
        return [tuple(t[-1:]) + (40,)], [1.5]
    if name == "seven":
        return ([(9,), (t[-1], 9), (t[-1], 40), (t[-2], t[-1], 41), tuple(t) + (eot - 1,), tuple(t[1:]) + (5, 0), (eot + 1, 9)],
                [0.25, 1e8, -INF, 2.0, -1e8, 3.0, -0.5])
    if name == "ctx7":
        return ([(t[-1], 9), (t[-1], 40), (t[-2], t[-1], 41), tuple(t) + (eot - 1,), tuple(t[1:]) + (5, 0), (eot + 1, 9), (1, 2, 3, 4)],
                [1e8, -INF, 2.0, -1e8, 3.0, -0.5, 1.0])
    if name == "deep":
        ids = [0, 31, 32, 63, 64, eot - 1] + [100 + 7 * i for i in range(122)]
        seqs = [tuple(t[31 - c:]) + (i,) for c in range(32) for i in ids]
        bias = (rng.standard_normal(len(seqs)) * 3).astype(np.float32)
        bias[[5, 700, 4000]] = -INF                                  # three banned ids for the rows their entries match
        return seqs, [float(b) for b in bias]
    assert name == "wide"
    n_ids = min(CAP, eot)
    ids = [int(i) for i in np.sort(rng.permutation(eot)[:n_ids])]
    per = CAP // n_ids
    ctxs = [(), tuple(t[-1:]), tuple(t[-2:]), tuple(t)][:per] if per > 1 else None
    seqs = [(ctxs[j] if ctxs else ((), tuple(t[-1:]))[i % 2]) + (i,) for i in ids for j in range(per)]
    bias = (rng.standard_normal(len(seqs)) * 3).astype(np.float32)
    bias[::97] = -INF
    return seqs, [float(b) for b in bias]


@functools.lru_cache(maxsize=None)
def want_state(V, name, h, k):
    seqs, bias = table(V, name)
    return SB.state(SB.expand(seqs, bias, eot=EOTS[V], V=V), hist(V, h, k), V)


def state_call(dbg, seq, pos, n_prompt, V, seqs, bias, boost=None, eot=None):
    n_ctx, B = seq.shape
    words = RR.words_of(V)
    toks, offs, bs, fl = SB.pack(seqs, bias, boost)
    hit, ban = np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32)
    cnt, ids, tot = np.zeros(B, np.int32), np.zeros((B, CAP), np.int32), np.zeros((B, CAP), np.float32)
    woff = np.zeros((B, words), np.int32)
    rc = dbg.lib.wmdbg_seqbias_state(dbg.handle, P(np.ascontiguousarray(seq, np.int32)), B, n_ctx, pos, n_prompt, V, P(toks), P(offs),
                                     P(bs), P(fl), len(seqs), EOTS[V] if eot is None else eot, P(hit), P(ban), P(cnt), P(ids), P(tot), P(woff))
    assert rc == 0, err_msg(dbg)
    return hit, ban, cnt, ids, tot, woff


def check_row(got, b, want, tag):
    hit, ban, cnt, ids, tot, woff = got
    wh, wb, wi, wt, wo = want
    assert np.array_equal(hit[b], wh), tag
    assert np.array_equal(woff[b], wo), tag
    assert np.array_equal(ban[b], wb), tag
    assert cnt[b] == wi.size, tag
    assert np.array_equal(ids[b, :wi.size], wi) and np.array_equal(bits(tot[b, :wi.size]), bits(wt)), tag
    # behind the list nothing was written: the hook's 0xff fill is still there
    assert np.all(ids[b, wi.size:] == -1) and np.all(bits(tot[b, wi.size:]) == 0xFFFFFFFF), tag


def seq_for(V, hs, k, n_prompt=1):
    seq = np.full((N_CTX, len(hs)), 9, np.int32)          # the prompt holds 9, the single-token entry's id: it never counts
    for b, h in enumerate(hs):
        seq[n_prompt:n_prompt + k, b] = hist(V, h, k)
    return seq


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [1, 5, 17, 128])
def test_state_kernel_rebuilds_the_rows(dbg, B, V):
    """Every hit, ban and offset word, the count and every list element, exactly, for tables of 1, 7 and 4096 entries at k in {434, 32,
    31, 30, 2, 1, 0} generated tokens -- in that order on ONE context, so every call has a shorter history than the one before
    it (a stale bit or list element would show; the hook pre-fills the outputs with 0xff, so an unwritten word shows too) --,
    then the longest one again with the rows permuted.  Rows: the history every entry of `deep` matches, one that matches
    none of the contexts, random ones, ids around eot, the last id of the vocabulary."""
    hs = [(b * 3 + B) % 8 for b in range(B)]
    names = ["one", "seven", "ctx7", "deep", "wide"] if B in (5, 17) else ["seven", "deep", "wide"]
    for name in names:
        seqs, bias = table(V, name)
        for k in (434, 32, 31, 30, 2, 1, 0) if B in (5, 17) or name == "seven" else (434, 31, 0):
            got = state_call(dbg, seq_for(V, hs, k), k, 1, V, seqs, bias)
            for b in range(B):
                check_row(got, b, want_state(V, name, hs[b], k), (name, k, b, hs[b]))
    seqs, bias = table(V, "deep")
    perm = np.random.default_rng(B).permutation(B)
    got = state_call(dbg, seq_for(V, hs, 434)[:, perm], 434, 1, V, seqs, bias)
    for i, b in enumerate(perm):
        check_row(got, i, want_state(V, "deep", hs[b], 434), (i, b))


def test_the_tables_do_what_their_names_say():
    """Conditions on the inputs of the test above, from the restatement alone."""
    for V in (1024, 51865):
        seqs, bias = table(V, "deep")
        t = SB.expand(seqs, bias, eot=EOTS[V], V=V)
        assert len(t) == CAP and all(SB.matches(s, hist(V, 0, k)) for s, _ in t for k in (434, 31))        # every entry matches
        assert sum(SB.matches(s, hist(V, 1, 434)) for s, _ in t) == 128                                   # the context-free ones
        assert {len(s) for s, _ in t} == set(range(1, 33))
        _, wb, wi, wt, _ = want_state(V, "deep", 0, 434)
        assert wi.size == 128 and int(np.count_nonzero(wb)) >= 1 and np.isinf(wt).sum() == 3
        t7 = SB.expand(*table(V, "ctx7"), eot=EOTS[V], V=V)
        assert not any(SB.matches(s, hist(V, 2, k)) for s, _ in t7 for k in (434, 31, 2, 0))               # a row that matches nothing
        assert want_state(V, "ctx7", 2, 434)[2].size == 0 and want_state(V, "ctx7", 0, 434)[2].size >= 3
        tw = SB.expand(*table(V, "wide"), eot=EOTS[V], V=V)
        assert len(tw) in (CAP, 4000) and len({s[-1] for s, _ in tw}) == min(CAP, EOTS[V])
        assert want_state(V, "wide", 0, 434)[2].size == min(CAP, EOTS[V])
        # `seven`: the entries (9,) and (t[-1], 9) end in one id, summed in table order; (t[-1], 40) bans 40
        _, wb, wi, wt, _ = want_state(V, "seven", 0, 434)
        assert wi.tolist() == [9, 40, 41, EOTS[V] - 1] and wt[0] == np.float32(np.float32(0.25) + np.float32(1e8)) and wt[1] == -INF
        assert V - 1 in history_pool(V)[6]


def test_state_kernel_prompt_boost_and_the_last_word(dbg):
    """A longer prompt (the history starts behind it), a prompt position (k = 0: the single-token entries still match), boosted
    prefixes through the hook's own expansion, eot = V with an entry on id V - 1 (the last, partly valid bitmap word)."""
    V, B = 51865, 5
    pool = history_pool(V)
    seq = np.ascontiguousarray(pool[[0, 1, 2, 5, 7], :200].T)            # [200][5]
    t = tail(V)
    h0 = [int(x) for x in pool[0, :200]]
    phrase = tuple(h0[150:154])                                           # four tokens row 0 has generated in a row
    seqs = [phrase, (V - 1,), (h0[150], h0[151], 77), (h0[150], 5)]
    bias = [2.0, 0.75, -INF, 1.0]
    boost = [True, False, False, False]
    table_ = SB.expand(seqs, bias, boost, eot=V, V=V)
    assert [s for s, _ in table_] == [phrase, phrase[:1], phrase[:2], phrase[:3], (V - 1,), (h0[150], h0[151], 77), (h0[150], 5)]
    for n_prompt, pos in ((7, 150), (7, 151), (7, 152), (7, 3), (7, 6), (1, 199), (200, 199)):
        got = state_call(dbg, seq, pos, n_prompt, V, seqs, bias, boost, eot=V)
        for b in range(B):
            g = seq[n_prompt:pos + 1, b]
            check_row(got, b, SB.state(table_, g, V), (n_prompt, pos, b))
        assert got[0][0, RR.words_of(V) - 1] == np.uint32(1) << np.uint32((V - 1) & 31)
    got = state_call(dbg, seq, 151, 7, V, seqs, bias, boost, eot=V)       # row 0 has just generated phrase[:2]: its third token is boosted
    assert got[3][0, :got[2][0]].tolist() == sorted({phrase[0], phrase[2], 77, V - 1}) and len(set(phrase)) == 4
    rc = dbg.lib.wmdbg_seqbias_state(dbg.handle, P(seq), B, 200, 5, 1, V, None, None, None, None, 0, V, *[P(a) for a in got])
    assert rc == 0 and not got[0].any() and not got[1].any() and not got[2].any() and not got[5].any()      # the empty table: nothing, written all the same


# =================================================================== B. the logits epilogue and the close
def with_table(dbg, seqs, bias, boost=None):
    """RK.run_step builds the wmdbg_step and calls dbg.lib.wmdbg_decode_close_rep(handle, step, penalty, ngram): this stand-in
    for `dbg` sends that call to wmdbg_decode_close_sb with the table behind it, so both tests share one set of operands."""
    toks, offs, bs, fl = SB.pack(seqs, bias, boost)
    keep = (toks, offs, bs, fl)

    def close_sb(handle, step, p, n):
        return dbg.lib.wmdbg_decode_close_sb(handle, step, p, n, P(keep[0]) if len(seqs) else None, P(keep[1]) if len(seqs) else None,
                                             P(keep[2]) if len(seqs) else None, P(keep[3]), len(seqs))
    lib = types.SimpleNamespace(wmdbg_decode_close_rep=close_sb, wmdbg_decode_close=dbg.lib.wmdbg_decode_close,
                                wm_last_error=dbg.lib.wm_last_error)
    return types.SimpleNamespace(lib=lib, handle=dbg.handle)


def step_table(w):
    """A table that decides on the histories of RK.step_inputs (logit bias: C 130 > A 114 > U0 72 > U1 50; row kinds by b % 3:
    0 ends in .. C A, 1 in .. A C, 2 in .. eot + 3, eot):
      kind 0: (A, C) bans C; (C, A, U0) lifts U0 to 72 + 50 + 60 = 182: U0
      kind 1: (C, U1) lifts U1 to 50 + 120 = 170 > 130: U1
      kind 2: (eot, U0) -- an id >= eot as context -- and the three-token entry through eot + 3 lift U0 to 72 + 50 + 30 + 1: U0
    and (U0,) adds 50 in every row, three entries end in U0 for kind 2 (the sum order), (U1, A) matches nowhere.  (The logits
    under the bias are N(0, 2^2): the margins above are >= 20.)"""
    A, C, U0, U1 = 20, 40, 27, w.eot - 1
    seqs = [(A, C), (U0,), (C, A, U0), (C, U1), (w.eot, U0), (w.eot + 3, w.eot, U0), (U1, A)]
    bias = [-INF, 50.0, 60.0, 120.0, 30.0, 1.0, 500.0]
    return seqs, bias, {0: U0, 1: U1, 2: U0}


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [3, 17])
def test_close_with_a_table_equals_the_restatement(dbg, B, V):
    """wmdbg_decode_close_sb against the restatement applied to the SAME hook's table-off logits, in the stated order -- the f32
    penalty first, then ONE f32 add of the total, the bans of both rules OR-ed --: the stored logits bit for bit (-inf at an id
    the table bans), the token the restatement's choice with the banned ids out of the allowed sets (at T = 0.7: arg-max of
    value * (1 / T) + Gumbel noise, a row whose two best scores lie within 1e-3 may take either -- at most one row of the test),
    the log-prob its f64 log-softmax over the allowed set within 1e-4 (the gate of
    test_logprobs_and_no_speech_against_the_oracle_and_the_gpus_own_logits), the next row the embedding of that token.
    Timestamp rules off and on.  An EMPTY table with the rules (1.0, 0) equals wmdbg_decode_close bit for bit everywhere, and
    with (1.3, 3) equals wmdbg_decode_close_rep; the table with (1.3, 3) equals the restatement of both."""
    w = RK.world(V)
    seq, pos, n_prompt, bias, C, _ = RK.step_inputs(w, B)
    seqs, sbias, want_tok = step_table(w)
    table_ = SB.expand(seqs, sbias, eot=w.eot, V=V)
    tsb, eot = w.ts_begin, w.eot
    ts_rng = np.array([(0, tsb, tsb + 3, V) if b % 2 == 0 else (eot, tsb, tsb + 3, V) for b in range(B)], np.int32)
    near = 0
    empty, full = with_table(dbg, [], []), with_table(dbg, seqs, sbias)
    for rng in (None, ts_rng):
        for T, seed, chunk0 in ((0.0, 0, 0), (0.7, 2 ** 40 + 7, 5)):
            kw = dict(seq=seq, pos=pos, n_prompt=n_prompt, bias=bias, T=T, seed=seed, chunk0=chunk0, rng=rng)
            off = RK.run_step(dbg, w, B, **kw)
            assert RK.same_step(off, RK.run_step(empty, w, B, rep=(1.0, 0), **kw)) is None
            assert RK.same_step(RK.run_step(dbg, w, B, rep=(1.3, 3), **kw), RK.run_step(empty, w, B, rep=(1.3, 3), **kw)) is None
            if T == 0.0 and rng is None:
                assert np.all(off.tok == C)                               # the plain decode would go on looping
            for p, n in ((1.0, 0), (1.3, 3)):
                r = RK.run_step(full, w, B, rep=(p, n), **kw)
                gi = pos + 1 - n_prompt
                for b in range(B):
                    g = seq[n_prompt:pos + 1, b]
                    row32, banned = RR.apply_rules(off.logits[b], g, p, n, eot)
                    row32, sbanned = SB.apply_bias(row32, table_, g)
                    banned = banned | sbanned
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
                    if T == 0.0 and rng is None and p == 1.0:             # the table decides, as step_table says
                        assert tok == want_tok[b % 3], (b, tok)
                assert r.logprob_written == B and np.all(bits(r.nospeech) == SENT32)
                assert np.array_equal(r.seq[pos + 1], r.tok) and np.array_equal(r.seq[:pos + 1], seq[:pos + 1])
                check_embedding(w, r, r.tok, pos, n_ctx=RK.STEP_CTX)
            # the first generated token: the history is empty, the single-token entry alone acts
            first = dict(kw, pos=n_prompt - 1)
            f_off, f_on = RK.run_step(dbg, w, B, **first), RK.run_step(full, w, B, rep=(1.3, 3), **first)
            for b in range(B):
                row32, _ = SB.apply_bias(f_off.logits[b], table_, [])
                assert np.array_equal(bits(f_on.logits[b]), bits(row32)) and row32[27] == np.float32(f_off.logits[b][27] + np.float32(50.0))
    assert near <= 1, near
