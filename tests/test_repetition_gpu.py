"""GPU tests of the repetition rules (wm_set_repetition_rules: repetition_penalty and no_repeat_ngram_size, DESIGN.md section
14) through every transcribe entry, on the `lively` tiny model of test_model_gpu.py and tones(4) -- a model whose plain greedy
decode falls into repetition loops.

The standard is the project's own-logits one (test_transcribe_options_gpu.py): the GPU's tokens are teacher-forced through
ctx.decode_logits, the existing filters and the numpy restatement (tests/repeat_ref.py) are applied to those rows, and the
arg-max must be the GPU's token at every position, the log-prob its log-softmax within 1e-4.

Tokens are NOT gated against the fp32 oracle (oracle/whisper_ref.py) here: measured on the CPU, 19-34 % of the positions
decoded under these rules lie within test_model_gpu._scaled_margin of a tie -- the rules remove the confident loop tokens and
leave the close calls --, so a bf16 product legitimately takes another branch and the histories part for good."""
import ctypes

import numpy as np
import pytest
import torch

import repeat_ref as RR
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
PROMPT = [1, 2, 3]
STOP = 1000                           # the eot of the loop measurements: ids 1000 .. 1023 are never penalised or banned
NEW = 32


def same(*arrays):
    a = arrays[0]
    return all(x.dtype == a.dtype and x.shape == a.shape and np.array_equal(x.view(np.uint8), a.view(np.uint8)) for x in arrays[1:])


def repeats(tokens, lens, n=3, eot=STOP):
    """repeated n-grams of every row of tokens [..., max_new] within its length"""
    t, l = np.asarray(tokens), np.asarray(lens)
    return [RR.repeated_ngrams(t[i][:l[i]], n, eot) for i in np.ndindex(l.shape)]


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(4))
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(4, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    w["xa"] = ctx.encode_mel(w["mel"])
    yield w
    ctx.set_repetition_rules()


def fresh(w):
    c = w["b"].Context(w["dims"])
    c.load_state_dict(w["sd_np"])
    c.finalize()
    return c


def test_off_is_off(world):
    """(a) Rules never set, set to (1.0, 0) and set-then-cleared: bit-identical tokens and log-probs, plain greedy included."""
    pcm = world["pcm"]
    c = fresh(world)
    try:
        g0 = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        r0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP)
        s0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
        for setup in (lambda: c.set_repetition_rules(1.0, 0, STOP), lambda: (c.set_repetition_rules(1.5, 3, STOP), c.set_repetition_rules())):
            setup()
            g = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
            r = c.transcribe(pcm, PROMPT, NEW, eot=STOP)
            s = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
            assert same(g0[0], g[0]) and same(g0[1], g[1])
            assert same(r0.tokens, r.tokens) and same(r0.lens, r.lens) and same(r0.logprobs, r.logprobs)
            assert same(s0.tokens, s.tokens) and same(s0.logprobs, s.logprobs)
    finally:
        c.close()


def test_no_repeat_ngram_through_every_entry(world):
    """(b) The plain decode has at least 5 repeated 3-grams in every row (asserted); with no_repeat_ngram_size = 3 the count is
    exactly 0 in every row of every entry: greedy, wm_transcribe at T = 0 and 0.8, wm_transcribe_mel, ragged prompts of 3 / 5 /
    9 tokens, every candidate of best_of = 3, every returned hypothesis of beam_size = 4, and wm_transcribe_windows."""
    ctx, pcm, mel_args = world["ctx"], world["pcm"], world["mel_args"]
    ctx.set_repetition_rules()
    plain = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
    print("plain greedy: repeated 3-grams per row", repeats(*plain), "distinct tokens", [len(set(t[:n])) for t, n in zip(*plain)])
    assert min(repeats(*plain)) >= 5, repeats(*plain)
    ragged = [[1, 2, 3], [7, 9, 1, 2, 3], [5, 5, 5, 5, 5, 5, 1, 2, 3], [4, 8, 1, 2, 3]]
    ctx.set_repetition_rules(1.0, 3, STOP)
    try:
        got = {}
        got["greedy"] = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        for T in (0.0, 0.8):
            r = ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            got["transcribe T=%g" % T] = (r.tokens, r.lens)
            r = ctx.transcribe_mel(*mel_args, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            got["mel T=%g" % T] = (r.tokens, r.lens)
        r = ctx.transcribe_mel(*mel_args, ragged, NEW, eot=STOP, sot_tail=3)
        got["ragged"] = (r.tokens, r.lens)
        r = ctx.transcribe_mel(*mel_args, ragged, NEW, eot=STOP, sot_tail=3, temperature=0.8, seed=5)
        got["ragged T=0.8"] = (r.tokens, r.lens)
        bo = ctx.transcribe_mel_best_of(*mel_args, PROMPT, NEW, 3, eot=STOP, temperature=0.8, seed=11)
        got["best_of"] = (bo.tokens, bo.lens)
        bm = ctx.transcribe_mel_beam(*mel_args, PROMPT, NEW, 4, eot=STOP)
        assert np.all(bm.n_hyp >= 1)
        got["beam"] = ([bm.tokens[b, h] for b in range(4) for h in range(bm.n_hyp[b])],
                       np.array([bm.lens[b, h] for b in range(4) for h in range(bm.n_hyp[b])]))
        bmr = ctx.transcribe_mel_beam(*mel_args, ragged, NEW, 4, eot=STOP, sot_tail=3)
        got["beam ragged"] = ([bmr.tokens[b, h] for b in range(4) for h in range(bmr.n_hyp[b])],
                              np.array([bmr.lens[b, h] for b in range(4) for h in range(bmr.n_hyp[b])]))
        with ctx.encode_windows(*mel_args) as ws:
            for T in (0.0, 0.8):
                r = ctx.transcribe_windows(ws, None, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
                got["windows T=%g" % T] = (r.tokens, r.lens)
            wb = ctx.transcribe_windows_beam(ws, None, PROMPT, NEW, 4, eot=STOP)
            assert same(wb.tokens, bm.tokens) and same(wb.lens, bm.lens)
        for name, (t, l) in got.items():
            assert repeats(t, l) == [0] * np.asarray(l).size, (name, repeats(t, l))
        # the entries that must agree do: greedy == wm_transcribe at T = 0, a window set == its mel windows
        assert same(got["greedy"][0], got["transcribe T=0"][0]) and same(got["greedy"][1], got["transcribe T=0"][1])
        for T in ("T=0", "T=0.8"):
            assert same(got["mel " + T][0], got["windows " + T][0]) and same(got["mel " + T][1], got["windows " + T][1]), T
        assert not same(got["greedy"][0], plain[0])
    finally:
        ctx.set_repetition_rules()


@pytest.mark.parametrize("ts_on", [False, True])
@pytest.mark.parametrize("rule", [(1.0, 3), (1.5, 0), (1.3, 3)])
def test_the_gpus_own_logits_under_the_rules_pick_the_gpus_tokens(world, rule, ts_on):
    """(c) The GPU's tokens teacher-forced through ctx.decode_logits; on those f32 rows the restatement (penalty in f32, banned
    ids to -inf), then the suppress lists and openai-whisper's timestamp filter: the arg-max is the GPU's token at EVERY
    position and |log-prob - log_softmax| <= 1e-4 (the gate of
    test_logprobs_and_no_speech_against_the_oracle_and_the_gpus_own_logits)."""
    ctx, pcm, xa = world["ctx"], world["pcm"], world["xa"]
    p, n = rule
    _rules(ctx, ts_on)
    ctx.set_repetition_rules(p, n, EOT)
    try:
        r = ctx.transcribe(pcm, PROMPT, NEW)
        g = ctx.transcribe_greedy(pcm, PROMPT, NEW)
        assert same(r.tokens, g[0])
        seqs = np.concatenate([np.tile(PROMPT, (4, 1)), r.tokens], axis=1)[:, :-1]
        own = ctx.decode_logits(seqs, xa)
        worst, touched, banned_n = 0.0, 0, 0
        for b in range(4):
            rows = np.array(own[b], dtype=np.float32, copy=True)
            for i in range(NEW):
                hist = r.tokens[b, :i]
                row, banned = RR.apply_rules(rows[len(PROMPT) - 1 + i], hist, p, n, EOT)
                touched += int(np.count_nonzero(row != rows[len(PROMPT) - 1 + i]))
                banned_n += int(banned.sum())
                row[banned] = -np.inf
                rows[len(PROMPT) - 1 + i] = row
            filt = _filtered_rows(rows, r.tokens[b], len(PROMPT), SPECIALS if ts_on else [], [EOT] if ts_on else [],
                                  (TS, EOT, MAXI) if ts_on else None)
            for i in range(NEW):
                tok = int(r.tokens[b, i])
                rg = filt[i][0]
                assert int(torch.argmax(rg)) == tok, (rule, ts_on, b, i, tok, int(torch.argmax(rg)))
                d = abs(float(torch.log_softmax(rg, 0)[tok]) - float(r.logprobs[b, i]))
                worst = max(worst, d)
                assert d <= 1e-4, (rule, ts_on, b, i, d)
            if n:
                assert RR.repeated_ngrams(r.tokens[b], n, EOT) == 0
        print("rule %s ts %s: worst |log-prob - own log-softmax| %.2e; penalised logits %d, banned ids %d" % (rule, ts_on, worst, touched, banned_n))
        assert (touched > 0) == (p != 1.0) and (banned_n > 0) == (n != 0)       # the rules had something to act on
    finally:
        ctx.set_repetition_rules()
        _rules(ctx, False)


def test_row_alone_lanes_and_greedy_agree(world):
    """(e) Under (1.3, 3): a row decoded alone equals the row among others, one lane equals three (24 rows: three groups of 8),
    wm_transcribe_greedy equals wm_transcribe at temperature 0 -- all bitwise."""
    ctx, pcm = world["ctx"], world["pcm"]
    ctx.set_repetition_rules(1.3, 3, STOP)
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
        assert repeats(res[0].tokens, res[0].lens) == [0] * 24
    finally:
        ctx.set_lanes(0)
        ctx.set_repetition_rules()


def test_changing_the_rules_between_calls_replays_the_same_graphs(world):
    """(f) Two calls on one context with different (p, n) -- the second replays the graphs the first captured: the parameters
    live in device memory -- each equal a fresh context's result; then rules off equals a fresh context that never had any."""
    ctx, pcm = world["ctx"], world["pcm"]
    try:
        got = []
        for p, n in ((1.5, 2), (1.2, 4), (1.0, 0), (2.0, 0)):
            ctx.set_repetition_rules(p, n, STOP)
            got.append(ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.0))
        assert not same(got[0].tokens, got[1].tokens)
        for (p, n), r in zip(((1.5, 2), (1.2, 4), (1.0, 0), (2.0, 0)), got):
            c = fresh(world)
            try:
                c.set_repetition_rules(p, n, STOP)
                w = c.transcribe(pcm, PROMPT, NEW, eot=STOP)
                assert same(w.tokens, r.tokens) and same(w.logprobs, r.logprobs) and same(w.lens, r.lens), (p, n)
                k = c.clone() if hasattr(c, "clone") else None     # a clone made later inherits the rules
                if k is not None:
                    try:
                        wk = k.transcribe(pcm, PROMPT, NEW, eot=STOP)
                        assert same(wk.tokens, r.tokens) and same(wk.logprobs, r.logprobs)
                    finally:
                        k.close()
            finally:
                c.close()
    finally:
        ctx.set_repetition_rules()


def test_invalid_arguments_and_the_f32_debug_path(world):
    """(g) WM_ERR_INVALID for a penalty that is not finite or <= 0, n outside [0, 32], eot outside [0, n_vocab]; the settings
    survive a refused call; the debug library's all-f32 precision path answers WM_ERR_STATE."""
    ctx, b, pcm = world["ctx"], world["b"], world["pcm"]
    V = world["dims"]["n_vocab"]
    fn = ctx.lib.wm_set_repetition_rules
    fn.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int32]
    try:
        ctx.set_repetition_rules(1.0, 3, STOP)
        want = ctx.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)
        for p, n, eot in ((float("nan"), 0, STOP), (float("inf"), 0, STOP), (0.0, 0, STOP), (-1.5, 3, STOP), (1e-39, 0, STOP), (1.5, -1, STOP),
                          (1.5, 33, STOP), (1.5, 3, -1), (1.5, 3, V + 1)):
            assert fn(ctx.handle, p, n, eot) == WM_ERR_INVALID, (p, n, eot)
            with pytest.raises(b.WhisperError) as e:
                ctx.set_repetition_rules(p, n, eot)
            assert e.value.status == WM_ERR_INVALID
        assert same(ctx.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)[0], want[0])
        for p, n, eot in ((1.5, 32, V), (0.5, 1, 0), (1.0, 0, V)):
            assert fn(ctx.handle, p, n, eot) == 0, (p, n, eot)
    finally:
        ctx.set_repetition_rules()
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_repetition_rules(1.0, 3, STOP)
        dbg.set_precision(True)
        with pytest.raises(b.WhisperError) as e:
            dbg.transcribe_greedy(pcm[:1], PROMPT, 4, eot=STOP)
        assert e.value.status == WM_ERR_STATE
        with pytest.raises(b.WhisperError) as e:
            dbg.set_repetition_rules(1.5, 0, STOP)
        assert e.value.status == WM_ERR_STATE
        dbg.set_repetition_rules()                       # switching them off is always allowed
        dbg.set_precision(False)
        dbg.set_repetition_rules(1.0, 3, STOP)
        assert repeats(*dbg.transcribe_greedy(pcm[:1], PROMPT, NEW, eot=STOP)) == [0]
    finally:
        dbg.close()
