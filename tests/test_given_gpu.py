"""GPU tests of given tokens (wm_set_given_tokens) through the transcribe entries, on the `lively` tiny
model of test_model_gpu.py (V = 1024) with the fixtures of tests/test_alternatives_gpu.py.  B = 5, 12 tokens.

Replay: the tokens of a call given back reproduce the call bit for bit -- the hand-over leaves the normaliser alone.  Other
text: the log-probs pass the project's own-logits standard (test_alternatives_gpu.py): the GPU's tokens are teacher-forced
through ctx.decode_logits, openai-whisper's filters are applied to those rows, and v(tok) - logsumexp(admissible) is compared
at 1e-4 (the gate of those files), with -inf exactly where the filters leave the id out."""
import ctypes

import numpy as np
import pytest
import torch

from test_alternatives_gpu import B, NEW, RAGGED, WM_ERR_INVALID, WM_ERR_STATE, mel_args
from test_constraint_gpu import CHOICES, above
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_repetition_gpu import STOP
from test_sampling_rules_gpu import PROMPT, fresh, same, same_result, world  # noqa: F401  (world: module fixture)
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WINDOW_ROWS = [6, 1, 3, 0, 2]


def given_of(tokens, lens):
    t, l = np.asarray(tokens), np.asarray(lens)
    return [[int(x) for x in t[i][:l[i]]] for i in np.ndindex(l.shape)]


def entries(w, T, eot, seed=11, given=None):
    """Every served kind of entry once, on the first B rows: plain, mel, ragged prompts, best-of 3, a window set, aligned.
    given: None, or per entry the table (a dict by entry name)."""
    ctx, ma = w["ctx"], mel_args(w)
    g = (lambda name: None) if given is None else (lambda name: given[name])
    kw = dict(eot=eot, temperature=T, seed=seed)
    out = {}
    out["transcribe"] = ctx.transcribe(w["pcm"][:B], PROMPT, NEW, no_speech_token=1000, given=g("transcribe"), **kw)
    out["mel"] = ctx.transcribe_mel(*ma, PROMPT, NEW, given=g("mel"), **kw)
    out["ragged"] = ctx.transcribe_mel(*ma, RAGGED, NEW, sot_tail=3, given=g("ragged"), **kw)
    out["best_of"] = ctx.transcribe_mel_best_of(*ma, PROMPT, NEW, 3, given=g("best_of"), **kw)
    with ctx.encode_windows(*mel_args(w, 8)) as ws:
        out["windows"] = ctx.transcribe_windows(ws, WINDOW_ROWS, PROMPT, NEW, given=g("windows"), **kw)
    out["aligned"] = ctx.transcribe_mel_aligned(*ma, PROMPT, NEW, given=g("aligned"), **kw)
    return out


class Config:
    """One setting of the context's other rules around a block of calls; .eot: the eot its calls take"""

    def __init__(self, w, kind):
        self.ctx, self.kind, self.b = w["ctx"], kind, w["b"]
        self.eot = STOP if kind == "constraint" else EOT

    def __enter__(self):
        if self.kind in ("rules", "rep_bias"):
            _rules(self.ctx, True)
        if self.kind == "rep_bias":
            self.ctx.set_repetition_rules(1.3, 3, EOT)
            self.ctx.set_sequence_bias({(17,): 1.5, (33, 34): 2.0, (40,): -np.inf}, eot=EOT)
        if self.kind == "constraint":
            above(self.ctx)
            self.ctx.set_constraint(self.b.constraint_from_choices(CHOICES), eot=STOP)
        return self

    def __exit__(self, *exc):
        self.ctx.set_constraint(None)
        self.ctx.set_sampling_rules()
        self.ctx.set_sequence_bias(None)
        self.ctx.set_repetition_rules()
        _rules(self.ctx, False)


def same_entry(a, b_, name):
    assert same_result(a, b_), name
    if name == "transcribe":
        assert same(a.no_speech_prob, b_.no_speech_prob)
    if name == "aligned":
        assert same(a.start_frames, b_.start_frames)
    if name == "best_of":
        assert same(a.best, b_.best)


@pytest.mark.parametrize("kind", ["plain", "rules", "rep_bias", "constraint"])
def test_replay_reproduces_the_call_bit_for_bit(world, kind):
    """The tokens of a temperature-0 call given back, lens for lens: tokens, lens, log-probs, no_speech_prob (start frames, the
    ranking) through every served entry."""
    with Config(world, kind) as cfg:
        off = entries(world, 0.0, cfg.eot)
        table = {name: given_of(r.tokens, r.lens) for name, r in off.items()}
        on = entries(world, 0.0, cfg.eot, given=table)
        for name in off:
            same_entry(on[name], off[name], name)
        assert int(off["mel"].lens.sum()) >= (B if kind == "constraint" else 40)


@pytest.mark.parametrize("kind", ["plain", "rules"])
def test_replay_of_a_sampled_call_at_any_temperature_seed_and_rules(world, kind):
    """The tokens of a T = 0.7 call replayed at T = 0 and at T = 0.7 under two seeds, without and with the sampling rules
    (8, 0.9, 0): the sampled call's tokens, lens and log-prob bits each time -- a given row never draws, and the normaliser is
    the temperature-1 one of the untruncated distribution."""
    ctx = world["ctx"]
    with Config(world, kind) as cfg:
        off = entries(world, 0.7, cfg.eot, seed=11)
        table = {name: given_of(r.tokens, r.lens) for name, r in off.items()}
        greedy = ctx.transcribe_mel(*mel_args(world), PROMPT, NEW, eot=cfg.eot)
        assert not same(greedy.tokens, off["mel"].tokens)                    # (the sampled call is not the greedy one)
        for T, seed, rule in ((0.0, 0, None), (0.7, 11, None), (0.7, 12345, None), (0.7, 11, (8, 0.9, 0.0)), (0.7, 99, (8, 0.9, 0.0))):
            ctx.set_sampling_rules(*(rule or ()))
            on = entries(world, T, cfg.eot, seed=seed, given=table)
            for name in off:
                assert same_result(on[name], off[name]), (name, T, seed, rule)


def other_texts(ts_on, seed=5):
    """B texts of NEW ids the model would not choose: seeded ids.  Under the rules rows 0 and 1 follow the timestamp grammar so
    that every id is admissible WHATEVER the sum rule decides -- an opening timestamp, then (text, a closed pair of equal
    timestamps) repeated: text stands only where the rules allow no timestamp, so the rule has nothing to force -- and the other
    rows break it: text in front of the first timestamp, a suppressed special, a timestamp past max_initial_timestamp."""
    g = np.random.default_rng(seed)
    texts = [[int(x) for x in g.integers(0, EOT, NEW)] for _ in range(B)]
    if ts_on:
        for b, ts in ((0, (2, 5, 9, 12, 20)), (1, (1, 3, 4, 30, 31))):
            t = texts[b]
            texts[b] = [TS + ts[0], t[1], TS + ts[1], TS + ts[1], t[4], TS + ts[2], TS + ts[2], t[7], TS + ts[3], TS + ts[3], t[10],
                        TS + ts[4]]
        texts[2][3], texts[2][6] = TS + 50, EOT + 3                                    # a timestamp, a suppressed special
        texts[3][0] = TS + MAXI + 5                                                    # past max_initial_timestamp
        texts[3][4], texts[4][2] = EOT + 1, EOT + 5                                    # (rows 2 .. 4: six ids that are never admissible)
    else:
        texts[2][3], texts[3][5] = TS + 50, 1023
    return texts


@pytest.mark.parametrize("ts_on", [False, True], ids=["rules_off", "rules_on"])
def test_another_texts_logprobs_against_the_gpus_own_logits(world, ts_on):
    ctx, xa = world["ctx"], world["xa"]
    texts = other_texts(ts_on)
    _rules(ctx, ts_on)
    try:
        plain = ctx.transcribe(world["pcm"][:B], PROMPT, NEW, eot=EOT if ts_on else -1)
        r = ctx.transcribe(world["pcm"][:B], PROMPT, NEW, eot=EOT if ts_on else -1, given=texts, alternatives=3)
    finally:
        _rules(ctx, False)
    assert same(r.tokens, np.array(texts, np.int32)) and np.all(r.lens == NEW) and not same(r.tokens, plain.tokens)
    seqs = np.concatenate([np.tile(PROMPT, (B, 1)), r.tokens], axis=1)[:, :-1]
    own = ctx.decode_logits(seqs, xa[:B])
    n_fin = n_inf = 0
    worst = 0.0
    for b in range(B):
        rows = np.array(own[b], dtype=np.float32, copy=True)
        filt = _filtered_rows(rows, r.tokens[b], len(PROMPT), SPECIALS if ts_on else [], [EOT] if ts_on else [],
                              (TS, EOT, MAXI) if ts_on else None)
        for i in range(NEW):
            if abs(filt[i][2]) < 1e-3:       # a sum-rule near-tie: either allowed set is right; not restated here
                continue
            row, tok = filt[i][0], int(r.tokens[b, i])
            got = float(r.logprobs[b, i])
            if not torch.isfinite(row).any():
                continue
            # entry 0 of the alternatives is what the model preferred: the arg-max of the row's admissible set
            assert abs(float(row[int(r.alt_tokens[b, i, 0])]) - float(row.max())) <= 1e-4, (b, i)
            if row[tok] == float("-inf"):
                assert got == -np.inf, (b, i, tok, got)
                n_inf += 1
            else:
                want = float(torch.log_softmax(row, 0)[tok])
                assert np.isfinite(got), (b, i, tok, got, want)
                worst = max(worst, abs(got - want))
                n_fin += 1
    print("ts %s: %d finite log-probs (max |d| %.3g), %d at -inf" % (ts_on, n_fin, worst, n_inf))
    assert worst <= 1e-4 and n_fin >= (20 if ts_on else B * NEW - 2)
    assert n_inf >= (5 if ts_on else 0)


def test_a_prefix_then_free_decode_is_the_call_on_the_longer_prompt(world):
    """openai-whisper's `prefix`: 4 given tokens, then the row decodes freely -- from index 4 on, the tokens of the plain call
    whose prompt ends in those 4 tokens (log-probs at 1e-4: the prompt's positions are other launches)."""
    ctx, ma = world["ctx"], mel_args(world)
    g = np.random.default_rng(8)
    pre = [[int(x) for x in g.integers(0, EOT, 4)] for _ in range(B)]
    r = ctx.transcribe_mel(*ma, PROMPT, NEW, given=pre)
    long_prompt = [PROMPT + p for p in pre]
    want = ctx.transcribe_mel(*ma, long_prompt, NEW - 4)
    assert same(r.tokens[:, :4], np.array(pre, np.int32))
    assert same(np.ascontiguousarray(r.tokens[:, 4:]), want.tokens)
    assert np.abs(r.logprobs[:, 4:] - want.logprobs).max() <= 1e-4
    free = ctx.transcribe_mel(*ma, PROMPT, NEW)
    assert not same(r.tokens, free.tokens)


def test_free_rows_of_a_mixed_call_a_row_alone_lanes_and_a_fresh_context(world):
    """Rows with lens = 0 equal the call without a table bit for bit; a given row's bits do not depend on the other rows, the
    lanes (the call's rows cut into as many decode groups, some without a given row) or what the context ran before."""
    ctx, pcm = world["ctx"], world["pcm"][:B]
    texts = other_texts(True)
    table = [texts[0], [], texts[2][:5], [], []]
    _rules(ctx, True)
    try:
        plain = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
        base = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table)
        for b in (1, 3, 4):
            assert same(base.tokens[b], plain.tokens[b]) and same(base.lens[b], plain.lens[b]) and same(base.logprobs[b], plain.logprobs[b])
        assert base.tokens[0].tolist() == texts[0] and base.tokens[2, :5].tolist() == texts[2][:5]
        empty = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, given=[[]] * B)       # a table of free rows: the plain call
        assert same_result(empty, plain)
        for lanes in (1, 2, 3):
            ctx.set_lanes(lanes)
            try:
                assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table), base), lanes
            finally:
                ctx.set_lanes(0)
        for idx in (slice(0, 1), slice(2, 3), slice(0, 3)):
            r = ctx.transcribe(pcm[idx], PROMPT, NEW, eot=EOT, given=table[idx])
            assert same(r.tokens, base.tokens[idx]) and same(r.lens, base.lens[idx]) and same(r.logprobs, base.logprobs[idx])
        clone = fresh(world)
        try:
            _rules(clone, True)
            assert same_result(clone.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table), base)
        finally:
            clone.close()
    finally:
        _rules(ctx, False)


def test_score_given_through_best_of_is_three_plain_calls_and_ranks_like_rank_candidates(world):
    ctx, b = world["ctx"], world["b"]
    g = np.random.default_rng(21)
    texts = [[[int(x) for x in g.integers(0, EOT, n)] for n in lens] for lens in ((3, 7, 5), (6, 6, 2), (1, 4, 9), (8, 3, 3))]
    rows = [5, 0, 2, 7]
    with ctx.encode_windows(*mel_args(world, 8)) as ws:
        out = b.score_given(ctx, ws, rows, PROMPT, texts, EOT, length_penalty=0.6, alternatives=2)
        for k in range(3):
            given = [t[k] + [EOT] for t in texts]
            p = ctx.transcribe_windows(ws, rows, PROMPT, 10, eot=EOT, budgets=[len(x) for x in given], given=given)
            for w_ in range(4):
                n = len(given[w_])
                assert p.lens[w_] == n and p.tokens[w_, :n].tolist() == given[w_]
                assert same(out.logprobs[w_][k], np.ascontiguousarray(p.logprobs[w_, :n])), (w_, k)
        uneven = [texts[0][:1], texts[1], texts[2][:2], texts[3][1:]]
        flat = b.score_given(ctx, ws, rows, PROMPT, uneven, EOT)
        assert flat.best is None
        assert same(flat.logprobs[0][0], out.logprobs[0][0]) and same(flat.logprobs[1][2], out.logprobs[1][2])
        assert same(flat.logprobs[3][0], out.logprobs[3][1])
    res = out.result
    assert res.lens.tolist() == [[len(t) + 1 for t in ts] for ts in texts]
    best, _ = b.rank_candidates(res.tokens, res.lens, res.logprobs, EOT, 0.6)
    assert same(out.best, best)
    for w_ in range(4):
        for k in range(3):
            assert abs(out.sum_logprob[w_][k] - float(np.sum(out.logprobs[w_][k], dtype=np.float64))) == 0
            assert out.avg_logprob[w_][k] == out.sum_logprob[w_][k] / (len(texts[w_][k]) + 1)
            assert out.alt_tokens[w_][k].shape == (len(texts[w_][k]) + 1, 2) and np.all(out.alt_counts[w_][k] == 2)


def test_the_table_is_consumed_and_refused_entries_answer_state(world, pkg):
    ctx, b, pcm, ma = world["ctx"], world["b"], world["pcm"][:B], mel_args(world)
    want = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
    table = [[7, 8, 9]] * B
    r = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table)
    assert r.tokens[:, :3].tolist() == [[7, 8, 9]] * B
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)          # consumed: the next call is the plain one
    ctx.set_given_tokens(table)
    ctx.set_given_tokens(None)                                                   # dropped: not served
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)

    def refused(call, c=ctx, n=B, status=WM_ERR_STATE):
        c.set_given_tokens([[7, 8, 9]] * n)
        with pytest.raises(b.WhisperError) as e:
            call()
        assert e.value.status == status, e.value
        assert "given" in str(e.value)
        if c is ctx:
            assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)  # consumed by the refused call

    refused(lambda: ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT))
    refused(lambda: ctx.transcribe_mel_beam(*ma, PROMPT, NEW, 1, eot=EOT))
    refused(lambda: ctx.transcribe_mel_beam(*ma, PROMPT, NEW, 3, eot=EOT), n=3 * B)
    refused(lambda: ctx.transcribe_mel_beam_aligned(*ma, PROMPT, NEW, 2, eot=EOT))
    refused(lambda: ctx.transcribe_mel_best_of_aligned(*ma, PROMPT, NEW, 2, eot=EOT, temperature=0.5), n=2 * B)
    with ctx.encode_windows(*ma) as ws:
        refused(lambda: ctx.transcribe_windows_beam(ws, None, PROMPT, NEW, 2, eot=EOT))
        refused(lambda: ctx.transcribe_windows_best_of_aligned(ws, None, PROMPT, NEW, 1, eot=EOT))
    draft = fresh(world)
    try:
        refused(lambda: ctx.transcribe_mel_speculative(draft, *ma, PROMPT, NEW, 3, eot=EOT))
    finally:
        draft.close()
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_precision(True)
        refused(lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT), c=dbg)
        dbg.set_precision(False)
        assert same_result(dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table), r)   # the debug library's product path serves it
    finally:
        dbg.close()
    from oracle import whisper_ref as R_
    multi = b.MultiContext(dict(R_.TINY_DIMS), devices=[0])
    try:
        multi.init_synthetic(11)
        prompt = [10, 21, 5, 7]
        t0, l0 = multi.transcribe_greedy(pcm, prompt, 6)
        multi.device_ctx(0).set_given_tokens([[7]] * B)
        with pytest.raises(b.WhisperError) as e:
            multi.transcribe_greedy(pcm, prompt, 6)
        assert e.value.status == WM_ERR_STATE
        t1, l1 = multi.transcribe_greedy(pcm, prompt, 6)                         # consumed: the next call is the plain one
        assert same(t1, t0) and same(l1, l0)
    finally:
        multi.close()
    with pytest.raises(ValueError):                                              # the wrappers refuse before any library call
        ctx.transcribe_mel(*ma, PROMPT, NEW, beam_size=2, given=table)
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)


def test_invalid_arguments(world):
    """WM_ERR_INVALID from the setter for an id outside the vocabulary, a lens entry outside [0, stride], null pointers or a
    stride below 1 with n > 0 -- and the pending table is gone; from the CALL for a table of another row count and a lens entry
    above max_new -- and that call still consumes the table."""
    ctx, b, pcm, V = world["ctx"], world["b"], world["pcm"][:B], world["V"]
    fn = ctx.lib.wm_set_given_tokens
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    want = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tok = np.full((B, 4), 7, np.int32)
    lens = np.full(B, 4, np.int32)

    def put(t=tok, stride=4, l=lens, n=B):
        return fn(ctx.handle, None if t is None else p(t), stride, None if l is None else p(l), n)
    high, neg = tok.copy(), tok.copy()
    high[2, 1], neg[4, 3] = V, -1
    long_, short = lens.copy(), lens.copy()
    long_[1], short[3] = 5, -1
    for bad in (dict(t=high), dict(t=neg), dict(l=long_), dict(l=short), dict(t=None), dict(l=None), dict(stride=0), dict(n=-1)):
        assert put() == 0                                                        # a good table pending ...
        assert put(**bad) == WM_ERR_INVALID, bad
        assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want), bad  # ... is gone with the refused one
    past = tok.copy()
    past[0, 3] = V + 5                                                           # behind a row's length: not read
    short = lens.copy()
    short[0] = 3
    assert put(t=past, l=short) == 0
    assert ctx.transcribe(pcm, PROMPT, NEW, eot=EOT).tokens[:, :3].tolist() == [[7, 7, 7]] * B
    for n, max_new in ((B - 1, NEW), (B + 1, NEW), (B, 3)):
        ctx.set_given_tokens([[7, 7, 7, 7]] * n)
        with pytest.raises(b.WhisperError) as e:
            ctx.transcribe(pcm, PROMPT, max_new, eot=EOT)
        assert e.value.status == WM_ERR_INVALID
        assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)      # consumed by the refused call
    ctx.set_given_tokens([[7]] * B)                                              # best-of: rows = B * best_of
    with pytest.raises(b.WhisperError) as e:
        ctx.transcribe_mel_best_of(*mel_args(world), PROMPT, NEW, 3, eot=EOT, temperature=0.5)
    assert e.value.status == WM_ERR_INVALID
    for bad in ([[-1]] * B, [[1.5]] * B, 5):
        with pytest.raises(ValueError):
            ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, given=bad)
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)
