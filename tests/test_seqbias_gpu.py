"""GPU tests of the sequence bias (wm_set_sequence_bias: bad words, biased sequences, boosted phrases)
through every transcribe entry, on the `lively` tiny model of test_model_gpu.py and tones(4), as test_repetition_gpu.py.

The standard is the project's own-logits one: the GPU's tokens are teacher-forced through ctx.decode_logits, the numpy
restatements (tests/repeat_ref.py, tests/seqbias_ref.py) and the existing filters are applied to those rows, and the arg-max
must be the GPU's token at every position, the log-prob its log-softmax within 1e-4.  Tokens are not gated against the fp32
oracle, for the reason test_repetition_gpu.py gives: near-ties under the rules."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import repeat_ref as RR
import seqbias_ref as SB
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_repetition_gpu import NEW, PROMPT, STOP, fresh, same
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
INF = float("inf")
RAGGED = [[1, 2, 3], [7, 9, 1, 2, 3], [5, 5, 5, 5, 5, 5, 1, 2, 3], [4, 8, 1, 2, 3]]


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(4))
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(4, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    w["xa"] = ctx.encode_mel(w["mel"])
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()
    w["plain"] = ctx.transcribe_greedy(w["pcm"], PROMPT, NEW, eot=STOP)
    yield w
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()


def ngrams_of(tokens, n, eot):
    """Counter of the n-grams of a token list that end in a text id"""
    t = [int(x) for x in tokens]
    return collections.Counter(tuple(t[i:i + n]) for i in range(len(t) - n + 1) if t[i + n - 1] < eot)


def bad_words(w):
    """Per row of the plain decode its most frequent 2-gram and 3-gram: the sequences to ban (each at least twice in its row)."""
    toks, lens = w["plain"]
    out = []
    for b in range(4):
        for n in (2, 3):
            seq, count = ngrams_of(toks[b][:lens[b]], n, STOP).most_common(1)[0]
            assert count >= 2, (b, n, seq, count)          # a condition on the inputs
            if seq not in out:
                out.append(seq)
    return out


def occurrences(tokens, lens, seqs):
    t, l = np.asarray(tokens), np.asarray(lens)
    return sum(SB.contains(t[i][:l[i]], s) for i in np.ndindex(l.shape) for s in seqs)


def test_off_is_off(world):
    """(a) Never set, set-then-cleared, n_seq = 0: bit-identical tokens and log-probs, plain greedy included.  And single-token
    entries leave no_speech_prob alone: it is read from the raw logits."""
    pcm = world["pcm"]
    c = fresh(world)
    try:
        g0 = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        r0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP, no_speech_token=5)
        s0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
        for setup in (lambda: c.set_sequence_bias({}, eot=STOP), lambda: (c.set_sequence_bias({(3, 4): -INF, (5,): 2.0}, eot=STOP), c.set_sequence_bias(None))):
            setup()
            g = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
            r = c.transcribe(pcm, PROMPT, NEW, eot=STOP, no_speech_token=5)
            s = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
            assert same(g0[0], g[0]) and same(g0[1], g[1])
            assert same(r0.tokens, r.tokens) and same(r0.lens, r.lens) and same(r0.logprobs, r.logprobs) and same(r0.no_speech_prob, r.no_speech_prob)
            assert same(s0.tokens, s.tokens) and same(s0.logprobs, s.logprobs)
        c.set_sequence_bias({(5,): 40.0, (int(r0.tokens[0, 0]),): -INF}, eot=STOP)      # the no-speech id boosted, a first token banned
        r = c.transcribe(pcm, PROMPT, NEW, eot=STOP, no_speech_token=5)
        assert same(r0.no_speech_prob, r.no_speech_prob) and not same(r0.tokens, r.tokens)
    finally:
        c.close()


def test_bad_words_through_every_entry(world):
    """(b) The most frequent 2- and 3-gram of every row of the plain decode (each at least twice in its row: asserted) banned:
    no row, candidate or hypothesis of any entry contains one -- greedy, wm_transcribe at T = 0 and 0.8, wm_transcribe_mel,
    ragged prompts of 3 / 5 / 9 tokens, every candidate of best_of = 3, every returned hypothesis of beam_size = 4, and
    wm_transcribe_windows."""
    ctx, pcm, mel_args = world["ctx"], world["pcm"], world["mel_args"]
    bad = bad_words(world)
    assert occurrences(*world["plain"], bad) >= 8
    ctx.set_sequence_bias({s: -INF for s in bad}, eot=STOP)
    try:
        got = {}
        got["greedy"] = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        for T in (0.0, 0.8):
            r = ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            got["transcribe T=%g" % T] = (r.tokens, r.lens)
            r = ctx.transcribe_mel(*mel_args, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            got["mel T=%g" % T] = (r.tokens, r.lens)
        r = ctx.transcribe_mel(*mel_args, RAGGED, NEW, eot=STOP, sot_tail=3)
        got["ragged"] = (r.tokens, r.lens)
        r = ctx.transcribe_mel(*mel_args, RAGGED, NEW, eot=STOP, sot_tail=3, temperature=0.8, seed=5)
        got["ragged T=0.8"] = (r.tokens, r.lens)
        bo = ctx.transcribe_mel_best_of(*mel_args, PROMPT, NEW, 3, eot=STOP, temperature=0.8, seed=11)
        got["best_of"] = (bo.tokens, bo.lens)
        bm = ctx.transcribe_mel_beam(*mel_args, PROMPT, NEW, 4, eot=STOP)
        assert np.all(bm.n_hyp >= 1)
        got["beam"] = ([bm.tokens[b, h] for b in range(4) for h in range(bm.n_hyp[b])],
                       np.array([bm.lens[b, h] for b in range(4) for h in range(bm.n_hyp[b])]))
        bmr = ctx.transcribe_mel_beam(*mel_args, RAGGED, NEW, 4, eot=STOP, sot_tail=3)
        got["beam ragged"] = ([bmr.tokens[b, h] for b in range(4) for h in range(bmr.n_hyp[b])],
                              np.array([bmr.lens[b, h] for b in range(4) for h in range(bmr.n_hyp[b])]))
        with ctx.encode_windows(*mel_args) as ws:
            for T in (0.0, 0.8):
                r = ctx.transcribe_windows(ws, None, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
                got["windows T=%g" % T] = (r.tokens, r.lens)
            wb = ctx.transcribe_windows_beam(ws, None, PROMPT, NEW, 4, eot=STOP)
            assert same(wb.tokens, bm.tokens) and same(wb.lens, bm.lens)
        for name, (t, l) in got.items():
            assert occurrences(t, l, bad) == 0, (name, occurrences(t, l, bad))
        assert same(got["greedy"][0], got["transcribe T=0"][0]) and same(got["greedy"][1], got["transcribe T=0"][1])
        for T in ("T=0", "T=0.8"):
            assert same(got["mel " + T][0], got["windows " + T][0]) and same(got["mel " + T][1], got["windows " + T][1]), T
        assert not same(got["greedy"][0], world["plain"][0])
    finally:
        ctx.set_sequence_bias(None)


def boost_table(ctx, xa, plain_tokens):
    """Positive entries from the decode WITHOUT the table (under the filters and repetition rules of the case): per row, at
    generated indices 2, 5, 9 and 14, the sequence (the two tokens in front, a TARGET that decode did not choose there), with a
    bias that lifts the target at least 8 above the row's best own text logit at that position (+ 0.31 |v|: the penalty of
    (1.3, 3) may shrink the target's own logit by that much).  -> {sequence: bias}"""
    seqs = np.concatenate([np.tile(PROMPT, (4, 1)), plain_tokens], axis=1)[:, :-1]
    own = ctx.decode_logits(seqs, xa)
    table = {}
    for b in range(4):
        for i in (2, 5, 9, 14):
            row = np.asarray(own[b][len(PROMPT) - 1 + i], np.float32)
            chosen = int(plain_tokens[b, i])
            target = (chosen + 17 + b) % (EOT - 1)
            assert target != chosen and target < EOT
            key = (int(plain_tokens[b, i - 2]), int(plain_tokens[b, i - 1]), target)
            if key not in table:
                table[key] = float(np.float32(row[:EOT].max() - row[target] + 8.0 + 0.31 * abs(row[target])))
    assert all(v > 0 and np.isfinite(v) for v in table.values())
    return table


@pytest.mark.parametrize("ts_on", [False, True])
@pytest.mark.parametrize("kind", ["boost", "boost+bans", "boost+bans+(1.3, 3)"])
def test_the_gpus_own_logits_under_the_table_pick_the_gpus_tokens(world, kind, ts_on):
    """(c) The GPU's tokens teacher-forced through ctx.decode_logits; on those f32 rows the restatements in the stated order
    (penalty, then v + total, bans of both rules to -inf), then the suppress lists and openai-whisper's timestamp filter: the
    arg-max is the GPU's token at EVERY position and |log-prob - log_softmax| <= 1e-4.  The positive entries take their
    contexts from the plain decode and target ids it did not choose; every row's tokens change (asserted)."""
    ctx, pcm, xa = world["ctx"], world["pcm"], world["xa"]
    p, n = (1.3, 3) if "(1.3, 3)" in kind else (1.0, 0)
    _rules(ctx, ts_on)
    try:
        ctx.set_repetition_rules(p, n, EOT)
        plain = ctx.transcribe(pcm, PROMPT, NEW)                    # the decode without the table
        table = dict(boost_table(ctx, xa, plain.tokens))
        if "bans" in kind:
            # a text id row 0 generates later on but no row generates among its first three tokens (so every row still reaches
            # its first boosted context), banned outright; and per row a 2-gram of the decode without the table
            early = {int(x) for x in plain.tokens[:, :3].ravel()} | {k[-1] for k in table}
            late = [int(x) for x in plain.tokens[0, 3:] if int(x) < EOT and int(x) not in early]
            table[(late[0] if late else next(i for i in range(EOT) if i not in early),)] = -INF
            for b in range(4):
                key = (int(plain.tokens[b, 20]), int(plain.tokens[b, 21]))
                if key[1] < EOT and key not in table:
                    table[key] = -INF
        ctx.set_sequence_bias(table, eot=EOT)
        ref = SB.expand(list(table), list(table.values()), eot=EOT, V=world["dims"]["n_vocab"])
        r = ctx.transcribe(pcm, PROMPT, NEW)
        g = ctx.transcribe_greedy(pcm, PROMPT, NEW)
        assert same(r.tokens, g[0])
        seqs = np.concatenate([np.tile(PROMPT, (4, 1)), r.tokens], axis=1)[:, :-1]
        own = ctx.decode_logits(seqs, xa)
        worst, biased, banned_n = 0.0, [0] * 4, 0
        for b in range(4):
            rows = np.array(own[b], dtype=np.float32, copy=True)
            for i in range(NEW):
                hist = r.tokens[b, :i]
                row, banned = RR.apply_rules(rows[len(PROMPT) - 1 + i], hist, p, n, EOT)
                row, sbanned = SB.apply_bias(row, ref, hist)
                biased[b] += int(any(np.isfinite(v) and v != 0 for v in SB.totals(ref, hist).values()))
                banned_n += int(sbanned.sum())
                row[banned | sbanned] = -np.inf
                rows[len(PROMPT) - 1 + i] = row
            filt = _filtered_rows(rows, r.tokens[b], len(PROMPT), SPECIALS if ts_on else [], [EOT] if ts_on else [],
                                  (TS, EOT, MAXI) if ts_on else None)
            for i in range(NEW):
                tok = int(r.tokens[b, i])
                rg = filt[i][0]
                assert int(torch.argmax(rg)) == tok, (kind, ts_on, b, i, tok, int(torch.argmax(rg)))
                d = abs(float(torch.log_softmax(rg, 0)[tok]) - float(r.logprobs[b, i]))
                worst = max(worst, d)
                assert d <= 1e-4, (kind, ts_on, b, i, d)
            assert not same(r.tokens[b], plain.tokens[b]), (kind, ts_on, b)          # the table changed the row
            for s, v in table.items():
                if v == -INF:
                    assert not SB.contains(r.tokens[b], s), (b, s)
        print("%s ts %s: worst |log-prob - own log-softmax| %.2e; positions with a finite total per row %s, banned ids %d"
              % (kind, ts_on, worst, biased, banned_n))
        assert min(biased) > 0 and (banned_n > 0) == ("bans" in kind)
    finally:
        ctx.set_sequence_bias(None)
        ctx.set_repetition_rules()
        _rules(ctx, False)


def test_a_boosted_phrase_is_its_hand_expanded_table(world):
    """(d) boost_prefixes against the table written out by hand, bitwise; two phrases that share their first token give it the
    MAXIMUM of the two biases, not the sum."""
    ctx, pcm = world["ctx"], world["pcm"]
    taken = {int(x) for x in world["plain"][0].ravel()}
    far = [i for i in range(100, STOP - 1) if i not in taken][:6]    # six text ids the plain decode never takes
    phrase = (far[0], far[1], far[2])
    other = (far[0], far[5])
    assert len(set(phrase)) == 3 and other[1] not in phrase
    run = lambda: ctx.transcribe(pcm, PROMPT, NEW, eot=STOP)        # noqa: E731
    # row 0's own logits at the first generated token: the larger bias lifts the shared first token 2 above the best id, so
    # its log-prob there is clearly below 0 with the maximum and clearly nearer to 0 with the sum (a condition on the inputs)
    row = np.asarray(ctx.decode_logits(np.tile(PROMPT, (4, 1)), world["xa"])[0][len(PROMPT) - 1], np.float32)
    hi = float(np.float32(row.max() - row[far[0]] + 2.0))
    lo = float(np.float32(0.5 * hi))
    assert hi > 2.0
    try:
        ctx.set_sequence_bias({phrase: hi}, boost=[phrase], eot=STOP)
        a = run()
        ctx.set_sequence_bias({phrase: hi, phrase[:1]: hi, phrase[:2]: hi}, eot=STOP)
        b = run()
        assert same(a.tokens, b.tokens) and same(a.logprobs, b.logprobs) and same(a.lens, b.lens)
        assert a.tokens[0, 0] == far[0] and not same(a.tokens, world["plain"][0])
        ctx.set_sequence_bias({phrase: lo, other: hi}, boost=[phrase, other], eot=STOP)
        two = run()
        ctx.set_sequence_bias({phrase: lo, phrase[:1]: hi, phrase[:2]: lo, other: hi}, eot=STOP)
        mx = run()
        ctx.set_sequence_bias({phrase: lo, phrase[:1]: float(np.float32(lo) + np.float32(hi)), phrase[:2]: lo, other: hi}, eot=STOP)
        sm = run()
        assert same(two.tokens, mx.tokens) and same(two.logprobs, mx.logprobs)
        assert two.tokens[0, 0] == far[0] and sm.tokens[0, 0] == far[0] and two.logprobs[0, 0] < sm.logprobs[0, 0] - 0.05
    finally:
        ctx.set_sequence_bias(None)


def mixed_table(w):
    bad = bad_words(w)
    t = {s: -INF for s in bad}
    first = [int(x) for x in w["plain"][0][:, 0]]
    t[((first[0] + 55) % (STOP - 1),)] = 3.0
    t.setdefault((bad[0][0], (bad[0][1] + 7) % (STOP - 1)), 12.0)
    return t


def test_row_alone_lanes_and_greedy_agree(world):
    """(e) Under a table of bans and biases: a row decoded alone equals the row among others, one lane equals three (24 rows),
    wm_transcribe_greedy equals wm_transcribe at temperature 0 -- all bitwise."""
    ctx, pcm = world["ctx"], world["pcm"]
    ctx.set_sequence_bias(mixed_table(world), eot=STOP)
    try:
        r = ctx.transcribe(pcm, PROMPT, NEW, eot=STOP)
        for b in (0, 3):
            one = ctx.transcribe(pcm[b:b + 1], PROMPT, NEW, eot=STOP)
            assert same(one.tokens[0], r.tokens[b]) and same(one.logprobs[0], r.logprobs[b]) and one.lens[0] == r.lens[b]
        g = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        assert same(g[0], r.tokens) and same(g[1], r.lens)
        big = np.tile(pcm, (6, 1))
        res = []
        for lanes in (1, 3):
            ctx.set_lanes(lanes)
            res.append(ctx.transcribe(big, PROMPT, NEW, eot=STOP, temperature=0.8, seed=9))
        assert same(res[0].tokens, res[1].tokens) and same(res[0].logprobs, res[1].logprobs) and same(res[0].lens, res[1].lens)
        t0 = ctx.transcribe(big, PROMPT, NEW, eot=STOP)
        assert same(t0.tokens, np.tile(r.tokens, (6, 1))) and same(t0.logprobs, np.tile(r.logprobs, (6, 1)))
        assert occurrences(res[0].tokens, res[0].lens, bad_words(world)) == 0
    finally:
        ctx.set_lanes(0)
        ctx.set_sequence_bias(None)


def test_changing_the_table_between_calls_replays_the_same_graphs(world):
    """(f) Two different tables on one context -- the second call replays the graphs the first captured: table and counts live in
    device memory -- each equal a fresh context's result (and a clone's made behind the set); then off equals a context that
    never had a table."""
    ctx, pcm = world["ctx"], world["pcm"]
    bad = bad_words(world)
    tables = [mixed_table(world), {bad[1]: -INF, (bad[0][0],): -2.0, bad[0]: 4.0}, None]
    try:
        got = []
        for t in tables:
            ctx.set_sequence_bias(t, eot=STOP)
            got.append(ctx.transcribe(pcm, PROMPT, NEW, eot=STOP))
        assert not same(got[0].tokens, got[1].tokens) and same(got[2].tokens, world["plain"][0])
        for t, r in zip(tables, got):
            c = fresh(world)
            try:
                if t is not None:
                    c.set_sequence_bias(t, eot=STOP)
                w = c.transcribe(pcm, PROMPT, NEW, eot=STOP)
                assert same(w.tokens, r.tokens) and same(w.logprobs, r.logprobs) and same(w.lens, r.lens)
                k = c.clone() if hasattr(c, "clone") else None     # a clone made later inherits the table
                if k is not None:
                    try:
                        wk = k.transcribe(pcm, PROMPT, NEW, eot=STOP)
                        assert same(wk.tokens, r.tokens) and same(wk.logprobs, r.logprobs)
                    finally:
                        k.close()
            finally:
                c.close()
    finally:
        ctx.set_sequence_bias(None)


def test_invalid_arguments_and_the_f32_debug_path(world):
    """(g) WM_ERR_INVALID for each rejected argument; a refused call leaves the previous table in force; the debug library's
    all-f32 precision path answers WM_ERR_STATE."""
    ctx, b, pcm = world["ctx"], world["b"], world["pcm"]
    V = world["dims"]["n_vocab"]
    fn = ctx.lib.wm_set_sequence_bias
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int32]
    fn.restype = ctypes.c_int

    def call(seqs, bias, boost=None, eot=STOP, offs=None):
        toks, o, bs, fl = SB.pack(seqs, bias, boost)
        o = o if offs is None else np.array(offs, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        return fn(ctx.handle, p(toks), p(o), p(bs), p(fl), len(seqs), eot)
    try:
        bad = bad_words(world)
        ctx.set_sequence_bias({s: -INF for s in bad}, eot=STOP)
        want = ctx.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)
        many = [(a, 10 + c, d) for a in range(10) for c in range(20) for d in range(20)]     # 4000 + 10 + 200 after expansion
        singles = [(i % 1000, i // 1000 + 1) for i in range(4097)]
        for args in (dict(seqs=[(V,)], bias=[1.0]), dict(seqs=[(-1, 2)], bias=[1.0]),          # a token outside the vocabulary
                     dict(seqs=[(1, STOP)], bias=[1.0]), dict(seqs=[(1, V - 1)], bias=[1.0]),   # a last token >= eot
                     dict(seqs=[(1,), ()], bias=[1.0, 1.0]),                                    # length 0
                     dict(seqs=[tuple([1] * 33)], bias=[1.0]),                                  # length 33
                     dict(seqs=[(1,)], bias=[float("nan")]), dict(seqs=[(1,)], bias=[INF]),     # NaN, +inf
                     dict(seqs=[(1, 2), (3,), (1, 2)], bias=[1.0, 1.0, 2.0]),                   # a duplicate
                     dict(seqs=[(1, 2)], bias=[-INF], boost=[True]),                            # -inf with boost_prefixes
                     dict(seqs=many, bias=[1.0] * 4000, boost=[True] * 4000),                   # 4210 entries after expansion
                     dict(seqs=singles, bias=[1.0] * 4097),                                     # 4097 given
                     dict(seqs=[(1, 2), (3,)], bias=[1.0, 1.0], offs=[0, 2, 1]),                # decreasing offsets
                     dict(seqs=[(1, 2), (3,)], bias=[1.0, 1.0], offs=[1, 2, 3]),                # offsets that do not start at 0
                     dict(seqs=[(1,)], bias=[1.0], eot=-1), dict(seqs=[(1,)], bias=[1.0], eot=V + 1)):
            assert call(**args) == WM_ERR_INVALID, {k: (v if k != "seqs" or len(v) < 9 else len(v)) for k, v in args.items()}
        with pytest.raises(b.WhisperError) as e:
            ctx.set_sequence_bias({(1, STOP): 1.0}, eot=STOP)
        assert e.value.status == WM_ERR_INVALID
        assert same(ctx.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)[0], want[0])              # the table in force stayed
        assert not same(want[0], world["plain"][0][:, :12])
        for args in (dict(seqs=many, bias=[1.0] * 4000), dict(seqs=singles[:4096], bias=[-INF] * 4096),
                     dict(seqs=[tuple([1] * 32)], bias=[1.0], boost=[True]), dict(seqs=[(V - 1, 0)], bias=[0.0], eot=V),
                     dict(seqs=[], bias=[], eot=0)):
            assert call(**args) == 0, len(args["seqs"])
        assert same(ctx.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)[0], world["plain"][0][:, :12])   # n_seq = 0: off
    finally:
        ctx.set_sequence_bias(None)
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_sequence_bias({(3, 4): -INF}, eot=STOP)
        dbg.set_precision(True)
        with pytest.raises(b.WhisperError) as e:
            dbg.transcribe_greedy(pcm[:1], PROMPT, 4, eot=STOP)
        assert e.value.status == WM_ERR_STATE
        with pytest.raises(b.WhisperError) as e:
            dbg.set_sequence_bias({(5,): 1.0}, eot=STOP)
        assert e.value.status == WM_ERR_STATE
        dbg.set_sequence_bias(None)                      # switching it off is always allowed
        dbg.set_precision(False)
        bad = bad_words(world)
        dbg.set_sequence_bias({s: -INF for s in bad}, eot=STOP)
        assert occurrences(*dbg.transcribe_greedy(pcm[:1], PROMPT, NEW, eot=STOP), bad) == 0
    finally:
        dbg.close()
