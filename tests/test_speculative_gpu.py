"""GPU tests of speculative decoding: wm_transcribe_mel_speculative.  The yardstick is the plain call -- every comparison is
array_equal on the raw bits of wm_transcribe_mel's tokens, lens, log-probs and no_speech_prob on the same context --, and for
the statistics the walk of tests/spec_ref.py over the same script of proposals.  Tiny geometry, the lively gain-4 synthetic
weights, windows of a few hundred frames, max_new <= 48."""
import ctypes
import math

import numpy as np
import pytest

import spec_ref as S
from oracle import whisper_ref as R
from test_model_gpu import tones

pytestmark = pytest.mark.gpu

TS, EOT, MAXI, NS_TOK = 900, 890, 20, 899          # the tiny vocabulary (1024): timestamps 900 .. 1023
SPECIALS = list(range(EOT + 1, TS))
PROMPT = [10, 21, 5]
NEW = 24
WM_ERR_INVALID, WM_ERR_STATE = 1, 3


def _model(pkg, seed, **over):
    dims = dict(R.TINY_DIMS, **over)
    c = pkg.binding.Context(dims, debug=True)
    c.init_synthetic(seed, matrix_gain=4.0)
    c.finalize()
    return c


@pytest.fixture(scope="module")
def models(pkg):
    """the target, a second context with the same weights, an unrelated draft (another seed, ONE decoder and encoder layer)"""
    tgt, same, other = _model(pkg, 11), _model(pkg, 11), _model(pkg, 5, n_text_layer=1, n_audio_layer=1)
    clone = tgt.clone()
    yield tgt, same, clone, other
    for c in (clone, other, same, tgt):
        c.close()


@pytest.fixture(scope="module")
def mel(models):
    return models[0].logmel(tones(5), out_dtype=np.float32)


def _rules(ctxs, on):
    for c in ctxs:
        if on:
            c.set_suppress(SPECIALS, [EOT])
            c.set_timestamp_rules(True, TS, EOT, MAXI)
        else:
            c.set_timestamp_rules(False)
            c.set_suppress([], [])


def _win(B):
    """B windows of 200 .. 440 frames at different seeks of the five recordings"""
    b = np.arange(B)
    return (b % 5).astype(np.int64) * 240000, 3000, (37 * b + 11).astype(np.int32), (200 + 60 * (b % 5)).astype(np.int32)


def _prompts(B, P=3):
    p = np.array(PROMPT + [7 + (3 * i) % 800 for i in range(P - 3)], dtype=np.int32)[:P]
    return np.ascontiguousarray(np.broadcast_to(p, (B, P)))


def _plain(pkg, ctx, mel, B, eot=-1, new=NEW, budgets=None, P=3):
    base, mlen, seek, nf = _win(B)
    opts = pkg.binding.wm_decode_opts(0.0, 0, NS_TOK, 0)
    return ctx.transcribe_mel_raw(mel, base, mlen, seek, nf, _prompts(B, P), new, eot, opts, logprobs=True, no_speech=True,
                                  budgets=budgets)


def _spec(ctx, draft, mel, B, k, eot=-1, new=NEW, budgets=None, P=3, script=None, T=0.0):
    base, mlen, seek, nf = _win(B)
    if script is not None:
        ctx.set_spec_script(script)
    return ctx.transcribe_mel_speculative(draft, mel, base, mlen, seek, nf, _prompts(B, P), new, k, eot=eot, temperature=T,
                                          no_speech_token=NS_TOK, budgets=budgets)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same(r, want, what):
    for name, x, y in zip(("tokens", "lens", "logprobs", "no_speech"), (r.tokens, r.lens, r.logprobs, r.no_speech_prob), want):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), (what, name)


def _tuning(ctx, key, value):
    ctx.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    assert ctx.lib.wmdbg_set_tuning(key.encode(), int(value)) == 0


def _walk(want, script, k, eot, new=NEW, budgets=None, P=3, spec_group=0, trace=None):
    toks, lens = want[0].tolist(), want[1].tolist()
    return S.walk(toks, lens, np.asarray(script).tolist(), P, new, k, eot, budgets, spec_group, trace)


# ---------------------------------------------------------------- 1. full acceptance
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("draft", ["same weights", "clone"])
def test_a_draft_with_the_targets_weights_has_every_proposal_accepted(pkg, models, mel, B, draft):
    tgt, same, clone, _ = models
    d = same if draft == "same weights" else clone
    want = _plain(pkg, tgt, mel, B)
    assert len({tuple(t) for t in want[0]}) == B or B == 1
    for k in (1, 3, 7):
        r = _spec(tgt, d, mel, B, k)
        _same(r, want, (draft, B, k))
        assert np.array_equal(r.accepted, r.proposed) and np.array_equal(r.kept, r.accepted), (k, r.stats)
        assert np.all(r.rounds == math.ceil((NEW - 1) / (k + 1))), (k, r.stats)
        assert np.all(r.proposed == NEW - 1 - r.rounds)      # every round gives its proposals and one token of the target's own


# ---------------------------------------------------------------- 2. an unrelated draft
@pytest.mark.parametrize("rules", [False, True])
def test_an_unrelated_draft_changes_the_rounds_and_nothing_else(pkg, models, mel, rules):
    tgt, _, _, other = models
    _rules((tgt, other), rules)
    try:
        for eot in (-1, EOT):
            want = _plain(pkg, tgt, mel, 3, eot=eot)
            for k in (2, 7):
                r = _spec(tgt, other, mel, 3, k, eot=eot)
                _same(r, want, (rules, eot, k))
                assert np.all(r.rounds <= NEW - 1) and np.all(r.rounds >= 1) and np.all(r.kept <= r.accepted)
                assert np.all(r.accepted <= r.proposed)
    finally:
        _rules((tgt, other), False)


# ---------------------------------------------------------------- 3. scripted proposals
def _corrupt(tokens, where):
    """the plain call's tokens with the entries (row, generated index) of `where` replaced by another text id"""
    sc = np.array(tokens, dtype=np.int32)
    for b, i in where:
        sc[b, i] = (sc[b, i] + 1) % 800
    return sc


def test_scripted_proposals_give_the_walks_statistics(pkg, models, mel):
    tgt, _, _, other = models
    B, k = 3, 3
    want = _plain(pkg, tgt, mel, B)
    # round 1 proposes generated tokens 1 .. 3: window 0 misses at row 0; the group then stands at token 2, round 2 proposes
    # 2 .. 4: window 1 misses at row k - 1 = 2 (token 4); later rounds: window 2 twice, and rounds without a miss
    script = _corrupt(want[0], [(0, 1), (1, 4), (2, 11), (2, 12), (0, 20)])
    trace = []
    stats = _walk(want, script, k, -1, trace=trace)
    live_acc = [a for w, live, acc, n in trace for a, l in zip(acc, live) if l]
    assert 0 in live_acc and k - 1 in live_acc                                     # a miss at row 0, at row k - 1 ...
    assert any(all(a == w - 1 for a in acc) for w, live, acc, n in trace)          # ... and at no row
    r = _spec(tgt, other, mel, B, k, script=script)
    _same(r, want, "scripted")
    assert r.stats.tolist() == [list(s) for s in stats]
    assert np.any(r.kept < r.accepted)                                             # the lockstep cut took accepted tokens away
    # the script that is the plain call: every proposal accepted
    r = _spec(tgt, other, mel, B, k, script=want[0])
    _same(r, want, "scripted, no miss")
    assert np.array_equal(r.accepted, r.proposed) and r.stats.tolist() == [list(s) for s in _walk(want, want[0], k, -1)]


def test_a_window_that_stops_mid_panel_leaves_its_neighbours_alone(pkg, models, mel):
    """early stop on a token the windows reach at different places: the one that ends inside a panel is frozen, the others
    go on -- and the same with a script that proposes the stopping token early"""
    tgt, _, _, other = models
    B, k = 3, 3
    free = _plain(pkg, tgt, mel, B)[0]
    # the stopping token: one the windows reach at as many different places as possible, none at its first token

    def first(t):
        return [int(np.argmax(row == t)) if np.any(row == t) else NEW for row in free]
    stop_tok = max((int(t) for t in np.unique(free[:, 1:])), key=lambda t: (min(first(t)) >= 1, len(set(first(t))), -min(first(t))))
    want = _plain(pkg, tgt, mel, B, eot=stop_tok)
    assert 1 < want[1].min() < NEW, (stop_tok, want[1])                               # some window does stop, behind its first token
    for script in (want[0], _corrupt(want[0], [(0, 2), (2, 5)])):
        r = _spec(tgt, other, mel, B, k, eot=stop_tok, script=script)
        _same(r, want, "stop mid-panel")
        assert r.stats.tolist() == [list(s) for s in _walk(want, script, k, stop_tok)]
    early = np.array(want[0])
    early[:, 3] = stop_tok                                                          # proposed early: a miss wherever it is not the truth
    r = _spec(tgt, other, mel, B, k, eot=stop_tok, script=early)
    _same(r, want, "stop proposed early")
    assert r.stats.tolist() == [list(s) for s in _walk(want, early, k, stop_tok)]


# ---------------------------------------------------------------- 4. rules, budgets, the narrowed last round
def test_suppress_lists_and_timestamp_rules_on_both_models(pkg, models, mel):
    tgt, _, _, other = models
    _rules((tgt, other), True)
    try:
        B, k = 3, 3
        want = _plain(pkg, tgt, mel, B, eot=EOT)
        gen = want[0]
        # A timestamp the rules FORCE, closed by a panel row s >= 1: an opening timestamp (the token in front of it is text) must
        # be followed by a timestamp or eot (ApplyTimestampRules), and with the script that is the plain call every round has
        # k + 1 rows, generated token i >= 1 being row (i - 1) % (k + 1) of its round.
        forced = [(b, i) for b in range(B) for i in range(2, int(want[1][b]))
                  if gen[b, i - 1] >= TS and gen[b, i - 2] < TS and (gen[b, i] >= TS or gen[b, i] == EOT) and (i - 1) % (k + 1) >= 1]
        assert forced, gen
        for script in (gen, _corrupt(gen, [(0, 1), (1, 4), (2, 11)])):
            r = _spec(tgt, other, mel, B, k, eot=EOT, script=script)
            _same(r, want, "rules")
            assert r.stats.tolist() == [list(s) for s in _walk(want, script, k, EOT)]
        early = np.array(gen)
        early[:, 2] = EOT
        _same(_spec(tgt, other, mel, B, k, eot=EOT, script=early), want, "rules, eot proposed early")
        # the draft's own rules shape its proposals, never the result
        _rules((other,), False)
        _same(_spec(tgt, other, mel, B, k, eot=EOT), want, "rules on the target only")
    finally:
        _rules((tgt, other), False)


@pytest.mark.parametrize("eot", [-1, EOT])
def test_token_budgets_that_end_inside_a_panel(pkg, models, mel, eot):
    tgt, same, _, other = models
    _rules((tgt, other, same), True)
    try:
        B, k = 4, 3
        budgets = [1, k, k + 2, NEW]
        want = _plain(pkg, tgt, mel, B, eot=eot, budgets=budgets)
        assert want[1].tolist()[:3] == [1, k, k + 2] or eot >= 0
        for d, script in ((same, None), (other, None), (other, np.maximum(want[0], 0))):   # (eot < 0 pads with -1)
            r = _spec(tgt, d, mel, B, k, eot=eot, budgets=budgets, script=script)
            _same(r, want, ("budgets", eot))
            if script is not None:
                assert r.stats.tolist() == [list(s) for s in _walk(want, script, k, eot, budgets=budgets)]
            assert r.stats[0].tolist() == [0, 0, 0, 0]                              # a budget of 1: the plain first step ends it
        # the budgets were this call's: the next plain call has none
        _same(_spec(tgt, same, mel, B, k, eot=eot), _plain(pkg, tgt, mel, B, eot=eot), "budgets consumed")
    finally:
        _rules((tgt, other, same), False)


def test_a_call_that_fills_the_context_narrows_its_last_rounds(pkg, models, mel):
    tgt, same, _, other = models
    n_ctx = R.TINY_DIMS["n_text_ctx"]
    P = n_ctx - NEW                                                                 # n_prompt + max_new == n_text_ctx
    want = _plain(pkg, tgt, mel, 2, P=P)
    for k, d in ((7, same), (5, other)):
        r = _spec(tgt, d, mel, 2, k, P=P)
        _same(r, want, ("context end", k))
        assert r.rounds.max() <= NEW - 1 and np.all(r.proposed <= k * r.rounds)


# ---------------------------------------------------------------- 5. grouping
def test_results_do_not_depend_on_the_group_cut(pkg, models, mel):
    tgt, _, _, other = models
    B, k = 5, 3
    _rules((tgt, other), True)
    try:
        want = _plain(pkg, tgt, mel, B, eot=EOT)
        script = _corrupt(want[0], [(0, 1), (1, 4), (2, 11), (3, 3), (4, 9), (4, 10)])
        rounds = {}
        for g in (1, 2, 5):
            _tuning(tgt, "spec_group", g)
            r = _spec(tgt, other, mel, B, k, eot=EOT, script=script)
            _same(r, want, ("group", g))
            assert r.stats.tolist() == [list(s) for s in _walk(want, script, k, EOT, spec_group=g)]
            rounds[g] = r.rounds.tolist()
        assert rounds[1] != rounds[5]                                               # the cut does change the rounds
    finally:
        _tuning(tgt, "spec_group", 0)
        _rules((tgt, other), False)


# ---------------------------------------------------------------- 5b. groups as large as the product cuts them
def _win_many(B):
    """_win for any B: the seeks wrap inside the recordings (the same windows as _win up to B = 67)"""
    b = np.arange(B)
    return (b % 5).astype(np.int64) * 240000, 3000, ((37 * b + 11) % 2500).astype(np.int32), (200 + 60 * (b % 5)).astype(np.int32)


def _plain_many(pkg, ctx, mel, B):
    base, mlen, seek, nf = _win_many(B)
    opts = pkg.binding.wm_decode_opts(0.0, 0, NS_TOK, 0)
    return ctx.transcribe_mel_raw(mel, base, mlen, seek, nf, _prompts(B), NEW, EOT, opts, logprobs=True, no_speech=True)


def _spec_many(ctx, draft, mel, B, k, script=None):
    base, mlen, seek, nf = _win_many(B)
    if script is not None:
        ctx.set_spec_script(script)
    return ctx.transcribe_mel_speculative(draft, mel, base, mlen, seek, nf, _prompts(B), NEW, k, eot=EOT, no_speech_token=NS_TOK)


def _misses(trace, c, row, k):
    """the rounds of full width in which window c, live, missed at proposal `row`"""
    return sum(1 for w, live, acc, n in trace if w == k + 1 and live[c] and acc[c] == row)


def _corrupt_rows(want, windows, k):
    """the plain call's tokens with, in each window of `windows`, one wrong proposal that meets the verify step as proposal 0
    and one as proposal k - 1, the last one a panel of k + 1 rows compares (found by walking the call: where an index lands
    depends on every miss in front of it).  Returns the script and the (window, row) pairs that were placed."""
    script, placed = np.array(want[0], dtype=np.int32), []
    for c in windows:
        for row in sorted({0, k - 1}):
            trace = []
            _walk(want, script, k, EOT, trace=trace)
            before = _misses(trace, c, row, k)
            for i in range(1, int(want[1][c])):
                if script[c, i] != want[0][c, i]:
                    continue
                trial, trace = _corrupt(script, [(c, i)]), []
                _walk(want, trial, k, EOT, trace=trace)
                if _misses(trace, c, row, k) == before + 1:
                    script = trial
                    placed.append((c, row))
                    break
    return script, placed


@pytest.mark.parametrize("B,k", [(64, 1), (42, 2)])
def test_one_group_at_the_row_bound(pkg, models, mel, B, k):
    """B (k + 1) = 128 / 126 rows: ONE decode group as wide as a verify step can be, windows 6 .. 63 of a group included"""
    tgt, _, _, other = models
    assert S.spec_groups(B, k)[1] == [B] and (B + 1) * (k + 1) > S.DEC_MAXB
    _rules((tgt, other), True)
    try:
        want = _plain_many(pkg, tgt, mel, B)
        windows = [0, 5, 6, 31, 41, B - 1]
        script, placed = _corrupt_rows(want, windows, k)
        # every listed window whose transcript is long enough has both misses (k = 1: they are one)
        long_enough = [c for c in windows if want[1][c] >= 2 * (k + 1) + 2]
        assert len(long_enough) >= 3, want[1][windows]
        assert all((c, row) in placed for c in long_enough for row in {0, k - 1}), (placed, want[1][windows])
        r = _spec_many(tgt, other, mel, B, k, script=script)
        _same(r, want, ("row bound", B, k))
        assert r.stats.tolist() == [list(s) for s in _walk(want, script, k, EOT)]
        assert k == 1 or np.any(r.kept < r.accepted)      # (k = 1: the one token a cut leaves IS the accepted proposal)
    finally:
        _rules((tgt, other), False)


def test_several_groups_of_an_unrelated_draft(pkg, models, mel):
    tgt, _, _, other = models
    B, k = 130, 3
    assert S.spec_groups(B, k)[1] == [26] * 5
    _rules((tgt, other), True)
    try:
        want = _plain_many(pkg, tgt, mel, B)
        r = _spec_many(tgt, other, mel, B, k)
        _same(r, want, ("several groups", B, k))
        assert np.all(r.kept <= r.accepted) and np.all(r.accepted <= r.proposed) and np.all(r.rounds <= NEW - 1)
    finally:
        _rules((tgt, other), False)


# ---------------------------------------------------------------- 6. the accept and commit kernels alone
def _key(v, n):
    u = int(np.float32(v).view(np.uint32))
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (u << 32) | (0xFFFFFFFF - n)


def _accept(ctx, G, w, pos, P, max_new, eot, winners, proposals, done, budget=None, n_tiles=4, n_ctx=64):
    """stage a verify step whose row (c, s) has winner winners[c][s] (logit 3 + s / 8; every other tile's best is lower) and run
    the two launches"""
    vp, ip = ctypes.c_void_p, ctypes.c_int
    fn = ctx.lib.wmdbg_spec_accept
    fn.argtypes = [vp] + [ip] * 7 + [ctypes.c_int32] + [vp] * 12
    fn.restype = ip
    rows = G * w
    tm = np.zeros((rows, n_tiles), dtype=np.uint64)
    txt = np.zeros((rows, n_tiles, 2), dtype=np.float32)
    win = np.zeros((rows, n_tiles, 2), dtype=np.float32)
    for c in range(G):
        for s in range(w):
            r, t = c * w + s, winners[c][s]
            for tile in range(n_tiles):
                best = 3.0 + s / 8 if tile == t // 16 else 1.0 + tile / 16
                tm[r, tile] = _key(best, t if tile == t // 16 else tile * 16 + 5)
                txt[r, tile] = (best, 2.0)          # (max, sum exp(v - max)) of the tile
                win[r, tile] = (best, 0.0)
    seq = np.zeros((n_ctx, G), dtype=np.int32)
    seq[pos] = 1
    for c in range(G):
        for s in range(1, w):
            seq[pos + s, c] = proposals[c][s - 1]
    done = np.array(done, dtype=np.int32)
    bud = None if budget is None else np.array(budget, dtype=np.int32)
    lp = np.zeros((max_new, G), dtype=np.float32)
    stats = np.zeros((G, 4), dtype=np.int32)
    rnd, acc = np.zeros(2, dtype=np.int32), np.zeros(G, dtype=np.int32)
    dseq = np.zeros((n_ctx, G), dtype=np.int32)
    posd = np.zeros(2, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    assert fn(ctx.handle, G, w, n_tiles, pos, P, n_ctx, max_new, eot, p(bud), p(tm), p(txt), p(win), p(seq), p(done), p(lp), p(stats),
              p(rnd), p(acc), p(dseq), p(posd)) == 0, ctx.lib.wm_last_error()
    return seq, done, lp, stats, rnd, acc, dseq, posd


def test_accept_and_commit_kernels_alone(models):
    tgt = models[0]
    P, max_new, eot, pos = 4, 20, 40, 9
    # 2 windows x width 3, window 1 frozen: window 0 accepts its first proposal, misses the second
    winners, props = [[17, 33, 50], [20, 21, 22]], [[17, 9], [20, 21]]
    seq, done, lp, stats, rnd, acc, dseq, posd = _accept(tgt, 2, 3, pos, P, max_new, eot, winners, props, [0, 1])
    n, live, inc = S.spec_round(3, [1, 2], [1, 0], [-1, -1], [max_new - (pos + 1 - P)] * 2)
    assert n == 2 and acc.tolist() == [1, 2]
    assert seq[pos + 1:pos + 3, 0].tolist() == [17, 33] and seq[pos + 1:pos + 3, 1].tolist() == [eot, eot]   # frozen: padding
    assert done.tolist() == [0, 1] and rnd.tolist() == [1, pos + n] and posd.tolist() == [pos + n, pos + n]
    assert stats.tolist() == [list(i) for i in inc]
    assert dseq[pos + n].tolist() == seq[pos + n].tolist() and np.count_nonzero(dseq) == 2
    g0 = pos + 1 - P
    for i in range(2):    # log-prob = winner's logit - log-sum-exp of the staged partials (f32 on the device)
        vals = [3.0 + i / 8 if t == winners[0][i] // 16 else 1.0 + t / 16 for t in range(4)]
        lse = math.log(sum(2.0 * math.exp(v - max(vals)) for v in vals)) + max(vals)
        assert abs(float(lp[g0 + i, 0]) - (3.0 + i / 8 - lse)) < 1e-5
    assert np.all(lp[:, 1] == 0) and np.count_nonzero(lp[:, 0]) == 2
    # both live: the group advances by the smaller count; window 1's second token is the stop token -> done, padded after
    winners, props = [[17, 33, 50], [20, eot, 22]], [[17, 33], [20, eot]]
    seq, done, lp, stats, rnd, acc, dseq, posd = _accept(tgt, 2, 3, pos, P, max_new, eot, winners, props, [0, 0])
    n, live, inc = S.spec_round(3, [2, 2], [1, 1], [-1, 1], [max_new - g0] * 2)
    assert n == 3 and acc.tolist() == [2, 2] and live == [1, 0]
    assert seq[pos + 1:pos + 4, 0].tolist() == [17, 33, 50] and seq[pos + 1:pos + 4, 1].tolist() == [20, eot, eot]
    assert done.tolist() == [0, 1] and rnd.tolist() == [1, pos + 3] and stats.tolist() == [list(i) for i in inc]
    assert lp[g0 + 2, 1] == 0 and lp[g0 + 1, 1] != 0
    # a budget that ends inside the panel
    seq, done, lp, stats, rnd, acc, dseq, posd = _accept(tgt, 2, 3, pos, P, max_new, -1, winners, props, [0, 0], budget=[g0 + 2, 99])
    n, live, inc = S.spec_round(3, [2, 2], [1, 1], [-1, -1], [2, max_new - g0])
    assert n == 3 and live == [0, 1] and done.tolist() == [1, 0] and stats.tolist() == [list(i) for i in inc]
    assert seq[pos + 1:pos + 4, 0].tolist() == [17, 33, 0]
    # width 1: the target's own token, nothing proposed
    seq, done, lp, stats, rnd, acc, dseq, posd = _accept(tgt, 3, 1, pos, P, max_new, eot, [[17], [eot], [5]], [[], [], []], [0, 0, 1])
    n, live, inc = S.spec_round(1, [0, 0, 0], [1, 1, 0], [-1, 0, -1], [max_new - g0] * 3)
    assert n == 1 and seq[pos + 1].tolist() == [17, eot, eot] and done.tolist() == [0, 1, 1] and rnd.tolist() == [1, pos + 1]
    assert stats.tolist() == [list(i) for i in inc] and acc.tolist() == [0, 0, 0]


# ---------------------------------------------------------------- 7. errors
def test_rejections_leave_the_context_as_it_was(pkg, models, mel):
    tgt, same, _, other = models
    b = pkg.binding
    B, k = 2, 3
    want = _plain(pkg, tgt, mel, B)

    def still_plain(what):
        _same(b.TranscribeResult(*_plain(pkg, tgt, mel, B), -1), want, what)      # the plain call still gives its usual bits

    def rejected(status, text, check=True, **kw):
        with pytest.raises(b.WhisperError) as e:
            _spec(tgt, kw.pop("draft", same), mel, B, kw.pop("k", k), **kw)
        assert e.value.status == status and text in str(e.value), str(e.value)
        if check:
            still_plain(text)

    rejected(WM_ERR_INVALID, "speculative decoding verifies the greedy choice: temperature must be 0 (got 0.5)", T=0.5)
    rejected(WM_ERR_INVALID, "draft_len 0 outside [1, 7]", k=0)
    rejected(WM_ERR_INVALID, "draft_len 8 outside [1, 7]", k=8)
    rejected(WM_ERR_INVALID, "speculative decoding needs a draft context of its own", draft=tgt)
    wide = _model(pkg, 3, n_vocab=1040)
    try:
        rejected(WM_ERR_INVALID, "differ from the target's", draft=wide)
    finally:
        wide.close()
    tgt.set_repetition_rules(1.3, 0, EOT)
    try:
        rejected(WM_ERR_STATE, "speculative decoding does not support the repetition rules set on this context", check=False)
    finally:
        tgt.set_repetition_rules()
    still_plain("after the repetition rules")
    tgt.set_sequence_bias({(5, 6): -2.0}, eot=EOT)
    try:
        rejected(WM_ERR_STATE, "speculative decoding does not support the sequence bias set on this context", check=False)
    finally:
        tgt.set_sequence_bias(None)
    still_plain("after the sequence bias")
    tgt.set_precision(True)
    try:
        with pytest.raises(b.WhisperError) as e:
            _spec(tgt, same, mel, B, k)
        assert e.value.status == WM_ERR_STATE and "speculative decoding is not supported by the all-f32 precision path" in str(e.value)
    finally:
        tgt.set_precision(False)
    still_plain("after the f32 path")
    # a script for another shape is refused and cleared
    tgt.set_spec_script(np.zeros((B, NEW + 1), dtype=np.int32))
    with pytest.raises(b.WhisperError) as e:
        _spec(tgt, same, mel, B, k)
    assert e.value.status == WM_ERR_INVALID and "the proposal script was set for" in str(e.value)
    r = _spec(tgt, same, mel, B, k)
    _same(r, want, "after every rejection")
    assert np.array_equal(r.accepted, r.proposed)


# ---------------------------------------------------------------- 8. the C entry without the two extra outputs
@pytest.mark.parametrize("rules", [False, True])
def test_the_c_entry_with_both_extra_outputs_null(pkg, models, mel, rules):
    """token_logprobs_out and no_speech_prob_out NULL: the plain call then closes its steps with the arg-max kernel's plain
    variant, the speculative call always from the extended decode's partials -- the tokens and lengths are the same bits"""
    tgt, same, _, other = models
    b = pkg.binding
    B, k = 3, 3
    _rules((tgt, other, same), rules)
    try:
        base, mlen, seek, nf = _win(B)
        for eot, budgets in ((-1, None), (EOT, [NEW, 5, 9])):
            want = tgt.transcribe_mel_raw(mel, base, mlen, seek, nf, _prompts(B), NEW, eot, None, logprobs=False, no_speech=False,
                                          budgets=budgets)
            assert want[2] is None and want[3] is None
            for d in (same, other):
                if budgets is not None:
                    tgt.set_token_budgets(budgets)
                head, n = tgt._mel_rows(mel, base, mlen, seek, nf, b.WM_MEM_HOST)
                pr = _prompts(B)
                toks = np.full((B, NEW), -7, dtype=np.int32)
                lens = np.full(B, -7, dtype=np.int32)
                rc = tgt.lib.wm_transcribe_mel_speculative(tgt.handle, d.handle, *head, n, pr.ctypes.data_as(ctypes.c_void_p), pr.shape[1],
                                                           k, NEW, eot, None, toks.ctypes.data_as(ctypes.c_void_p),
                                                           lens.ctypes.data_as(ctypes.c_void_p), None, None, None, b.WM_MEM_HOST)
                assert rc == 0, tgt.lib.wm_last_error()
                assert np.array_equal(toks, want[0]) and np.array_equal(lens, want[1]), (rules, eot)
    finally:
        _rules((tgt, other, same), False)
