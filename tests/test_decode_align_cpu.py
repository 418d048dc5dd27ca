"""CPU tests of the host side of word timestamps from the decode's own pass: binding.decode_alignment_text on hand-made rows,
transcribe_long's word_timestamps="decode" -- its ValueErrors and, on the recording fake of tests/test_longform_calls_cpu.py,
its call sequence and words --, and the transcribe plan's optional bound on the rows of a group (wmdbg_tx_plan_bounded)
against the unbounded plan and tests/tx_plan_ref.py."""
import ctypes
import importlib
import itertools
import math

import numpy as np
import pytest

import tx_plan_ref as ref
from test_longform_calls_cpu import LANGS, SCRIPT, SECONDS, STD, RecCtx, _rec, make_vocab
from test_longform_words_cpu import EOT, NO_TS, TB
from test_tx_plan_cpu import B_ALL, LANES, PLAN_IN, PLAN_OUT, WIDTHS

B = importlib.import_module("openai_whisper_coreml_amd.binding")
IP = ctypes.POINTER(ctypes.c_int32)


# ---------------------------------------------------------------- decode_alignment_text
def _row(tokens, frames, lps, width=8):
    """a row of an AlignedResult: tokens padded with eot, start frames [len] + the window's end + -1 ..., log-probs"""
    n = len(tokens)
    t = np.full(width, EOT, dtype=np.int32)
    t[:n] = tokens
    sf = np.full(width + 1, -1, dtype=np.int32)
    sf[:n + 1] = frames
    lp = np.zeros(width, dtype=np.float32)
    lp[:n] = lps
    return t, n, sf, lp


def test_text_rows_with_timestamps_interleaved_and_a_stopping_eot():
    # <|0.00|> a b <|2.00|> <|2.00|> c <|3.00|> eot: the text is a b c, a timestamp's row closes a word
    toks = [TB, 5, 6, TB + 100, TB + 100, 7, TB + 150, EOT]
    frames = [0, 3, 40, 98, 100, 101, 149, 150, 1500]
    lps = [-0.5, math.log(0.25), math.log(0.5), -1.0, -1.0, math.log(0.125), -2.0, -3.0]
    t, n, sf, lp = _row(toks, frames, lps)
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT)
    assert text == [5, 6, 7]
    assert bounds.tolist() == [3, 40, 101, 149] and bounds.dtype == np.int32     # (the final one: the row behind token 7)
    assert np.allclose(probs, [0.25, 0.5, 0.125], rtol=1e-6, atol=0) and probs.dtype == np.float64
    # cut to the text a window's segments kept: the final boundary is again the row behind the last text token kept
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT, n_text=2)
    assert text == [5, 6] and bounds.tolist() == [3, 40, 98] and len(probs) == 2
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT, n_text=1)
    assert text == [5] and bounds.tolist() == [3, 40]
    with pytest.raises(ValueError):
        B.decode_alignment_text(t, n, sf, lp, EOT, n_text=4)


def test_text_rows_that_end_without_eot_and_rows_without_text():
    # a budget ended the row behind a text token: the final boundary is the window's end, start_frames[len]
    t, n, sf, lp = _row([5, 6], [10, 20, 617], [-1.0, -2.0])
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT)
    assert text == [5, 6] and bounds.tolist() == [10, 20, 617]
    assert np.allclose(probs, np.exp([-1.0, -2.0]), rtol=1e-6, atol=0)
    # tokens past the length are never looked at (they read eot, but a caller's buffer may hold anything)
    t[n:] = 3
    assert B.decode_alignment_text(t, n, sf, lp, EOT)[0] == [5, 6]
    # timestamps and eot only; nothing generated at all (all -1)
    t, n, sf, lp = _row([TB, TB + 50, EOT], [0, 0, 25, 1500], [-1.0] * 3)
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT)
    assert text == [] and bounds.tolist() == [0] and probs.shape == (0,)
    t, n, sf, lp = _row([], [-1], [])
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT)
    assert text == [] and bounds.tolist() == [-1] and probs.shape == (0,)
    # the one-token row of a prompt that ends in <|startoftranscript|>: (0, M)
    t, n, sf, lp = _row([9], [0, 1500], [math.log(0.5)])
    text, bounds, probs = B.decode_alignment_text(t, n, sf, lp, EOT)
    assert text == [9] and bounds.tolist() == [0, 1500] and np.allclose(probs, [0.5])


# ---------------------------------------------------------------- transcribe_long(word_timestamps="decode") on the fake
@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


class AlignedCtx(RecCtx):
    """RecCtx whose aligned entries return the scripted window's decode plus start frames made from its script: generated
    token k starts where the text token at or behind it starts (frames[text tokens in front of k]), the row ends at the last
    scripted frame; log-probs are the log of the scripted probabilities on text tokens."""

    def _aligned(self, r, ids, max_new):
        start = np.full((len(ids), max_new + 1), -1, dtype=np.int32)
        for i, sid in enumerate(ids):
            w = self.window(sid)
            n, seen = int(r.lens[i]), 0
            for k in range(n + 1):
                start[i, k] = w["frames"][min(seen, len(w["frames"]) - 1)]
                if k < n and r.tokens[i, k] < EOT:
                    if not w["skip"] and r.logprobs[i, k] > -1.0:     # (a kept attempt: -0.1 everywhere)
                        r.logprobs[i, k] = np.float32(math.log(w["probs"][min(seen, len(w["probs"]) - 1)]))
                    seen += 1
        return B.AlignedResult(r.tokens, r.lens, r.logprobs, r.no_speech_prob, EOT, start)

    def transcribe_mel_aligned(self, *a, **kw):
        self._log("transcribe_mel_aligned", a, kw)
        for b, s, sid in zip(a[1], a[3], kw["sample_ids"]):
            self.sid_of[(int(b), int(s))] = int(sid)
        return self._aligned(self._decode(kw["sample_ids"], a[6], kw), kw["sample_ids"], a[6])

    def transcribe_windows_aligned(self, *a, **kw):
        self._log("transcribe_windows_aligned", a, kw)
        for row, sid in zip(a[1], kw["sample_ids"]):
            a[0].sid[int(row)] = int(sid)
        return self._aligned(self._decode(kw["sample_ids"], a[3], kw), kw["sample_ids"], a[3])


def _run(ctx, **kw):
    return B.transcribe_long(ctx, [_rec(s) for s in SECONDS], **kw)


def _timing(out):
    return [[(s["seek"], s["start"], s["end"], s["tokens"], [(w["word"], w["start"], w["end"]) for w in s.get("words", [])])
             for s in o["segments"]] for o in out]


@pytest.mark.parametrize("reuse", [False, True])
def test_decode_mode_call_sequence_and_words_on_the_fake(vocab, reuse):
    """Every decode call of the run is the aligned entry with the arguments the plain entry gets under word_timestamps=True,
    no align* call is made, and -- the fake's start frames being the scripted ones in both modes -- the segments and word
    times are those of word_timestamps=True; the probabilities are exp(log-prob) of the same numbers."""
    kw = dict(STD, vocab=vocab, language=LANGS, reuse_encoder=reuse)
    a, t = AlignedCtx(SCRIPT), AlignedCtx(SCRIPT)
    got = _run(a, word_timestamps="decode", **kw)
    want = _run(t, word_timestamps=True, no_timestamps=NO_TS, **kw)
    plain, aligned = ("transcribe_windows", "transcribe_windows_aligned") if reuse else ("transcribe_mel", "transcribe_mel_aligned")
    names = [c[0] for c in a.calls]
    assert not [n for n in names if n.startswith("align")] and plain not in names and aligned in names
    assert any(n.startswith("align") for n in (c[0] for c in t.calls))
    # the same calls in the same order, the word step's alignment calls left out and the decode entries renamed
    rest = [c for c in t.calls if not c[0].startswith("align")]
    assert [[aligned if c[0] == plain else c[0]] + c[1:] for c in rest] == a.calls
    assert _timing(got) == _timing(want)
    assert [o["seeks"] for o in got] == [o["seeks"] for o in want]
    pg = [w["probability"] for o in got for s in o["segments"] for w in s.get("words", [])]
    pw = [w["probability"] for o in want for s in o["segments"] for w in s.get("words", [])]
    assert len(pg) > 0 and np.allclose(pg, pw, rtol=1e-6, atol=0)
    windows = [w for o in got for w in o["windows"]]
    assert any(len(w["temperatures"]) > 1 for w in windows) and any(w["skipped"] for w in windows)     # a fallback, a skip


def test_decode_mode_value_errors_come_before_any_library_call(vocab):
    for kw in (dict(word_timestamps="decode", vocab=vocab, best_of=2),
               dict(word_timestamps="decode", vocab=vocab, beam_size=2),
               dict(word_timestamps="decode", vocab=vocab, beam_size=2, best_of=3),
               dict(word_timestamps="decode"),                    # no vocab
               dict(word_timestamps="decoder", vocab=vocab),      # no such mode
               dict(word_timestamps="decode", vocab=vocab, hallucination_silence_threshold=-1.0)):
        ctx = AlignedCtx(SCRIPT)
        with pytest.raises(ValueError):
            _run(ctx, **dict(STD, **kw))
        assert ctx.calls == [], kw
    # no_timestamps is not needed, and the hallucination rules take the mode as word timestamps
    ctx = AlignedCtx(SCRIPT)
    out = _run(ctx, **dict(STD, word_timestamps="decode", vocab=vocab, hallucination_silence_threshold=2.0))
    assert any(s.get("words") for o in out for s in o["segments"])


# ---------------------------------------------------------------- the plan's bound on the rows of a group
@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_tx_plan.argtypes = [IP, ctypes.c_int, IP, IP, ctypes.c_int]
    lib.wmdbg_tx_plan_bounded.argtypes = [IP, IP, ctypes.c_int, IP, IP, ctypes.c_int]
    lib.wmdbg_tx_plan.restype = lib.wmdbg_tx_plan_bounded.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(IP)


def _grid(Ns, knobs):
    """tests/test_tx_plan_cpu.py's grid: per (N, lanes, explicit, prof_on) the inputs [n][12] and the restatement's plan"""
    inner = np.array(np.meshgrid(B_ALL, (0, 1), WIDTHS, *knobs, indexing="ij")).reshape(6, -1)
    for N, lanes, explicit, prof in itertools.product(Ns, LANES, (0, 1), (0, 1)):
        a = np.zeros((inner.shape[1], PLAN_IN), dtype=np.int32)
        a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4] = inner[0], N, lanes, explicit, prof
        a[:, 5:10] = inner[1:].T
        yield a, ref.plan(inner[0], N, lanes, explicit, prof, *inner[1:])


def _plans(dbg, a, bound):
    n = len(a)
    out = np.full((n, PLAN_OUT), -1, dtype=np.int32)
    cut = np.full(2 * int(a[:, 0].sum()) + 8, -1, dtype=np.int32)
    if bound is None:
        assert dbg.wmdbg_tx_plan(_p(a), n, _p(out), _p(cut), len(cut)) == n
    else:
        bounds = np.ascontiguousarray(np.broadcast_to(np.asarray(bound, dtype=np.int32), (n,)))
        assert dbg.wmdbg_tx_plan_bounded(_p(a), _p(bounds), n, _p(out), _p(cut), len(cut)) == n
    return out, cut


def test_without_a_bound_every_plan_of_the_grid_is_unchanged(dbg):
    done = 0
    for a, (L, parts, G, n_lanes, kind) in _grid((1, 2, 3, 5, 8), ((0, 1, 2, 3), (0, 8), (0, 4, 16))):
        want, want_cut = _plans(dbg, a, None)
        got, got_cut = _plans(dbg, a, 0)
        assert np.array_equal(got, want) and np.array_equal(got_cut, want_cut)
        for i, v in enumerate((L, parts, G, n_lanes, kind)):     # ... which is the restatement's
            assert np.array_equal(got[:, i], v), i
        done += len(a)
    assert done == 600 * 5 * 5 * 2 * 2 * 2 * 4 * 4 * 2 * 3


@pytest.mark.parametrize("bound", [1, 7, 48, 97, 128, 200])
def test_with_a_bound_no_group_exceeds_it_and_the_groups_stay_balanced(dbg, bound):
    for N in (1, 3):
        for a, (L, parts, G, n_lanes, kind) in _grid((N,), ((0, 2), (0,), (0,))):
            out, cut = _plans(dbg, a, bound)
            Bn = a[:, 0].astype(np.int64)
            Gb = out[:, 2].astype(np.int64)
            w_max = max(1, bound // N)                       # whole windows, at least one per group
            need = -(-Bn // w_max)
            assert (Gb >= need).all() and (Gb >= 1).all() and (Gb <= Bn).all()
            # a plan the bound does not bind is the unbounded plan
            free = -(-Bn // G) <= w_max
            assert np.array_equal(out[free, :5], _plans(dbg, a, None)[0][free, :5]) and np.array_equal(Gb[free], G[free])
            # parts are one group each: they stay only when they are enough
            assert ((out[:, 1] == 0) | (out[:, 1] >= need)).all()
            assert (out[:, 3] >= 1).all() and (out[:, 3] <= Gb).all()
            start = out[:, 5].astype(np.int64)
            for i in np.random.default_rng(bound).choice(len(a), size=400, replace=False):   # the cuts of a sample, in full
                g = int(Gb[i])
                b0, cg = cut[start[i]:start[i] + g], cut[start[i] + g:start[i] + 2 * g]
                assert cg.sum() == Bn[i] and cg.max() <= w_max and cg.max() - cg.min() <= 1 and cg.min() >= 1, (a[i, :10], bound)
                assert b0[0] == 0 and np.array_equal(b0[1:], np.cumsum(cg)[:-1])
    # the bound is refused below zero
    one = np.array([[40, 1, 3, 0, 0, 0, 384, 0, 0, 0, 0, 0]], dtype=np.int32)
    out, cut = np.zeros((1, PLAN_OUT), np.int32), np.zeros(16, np.int32)
    neg = np.array([-1], dtype=np.int32)
    assert dbg.wmdbg_tx_plan_bounded(_p(one), _p(neg), 1, _p(out), _p(cut), 16) == -1
