"""GPU tests of window sets through the C ABI: wm_windows_encode keeps the cross-attention K/V of a set of mel windows, and
wm_transcribe_windows / wm_transcribe_windows_beam / wm_align_windows / wm_windows_detect_language give, BIT FOR BIT, what
their mel counterparts give on the same windows -- in any row order, with repeats, across decode groups and lanes, from
clones, and whatever ran in between.  Then binding.transcribe_long(reuse_encoder=True) against the default run."""
import contextlib
import ctypes

import numpy as np
import pytest

from test_align_gpu import NO_TS, _text
from test_longform_gpu import SOT_PREV, _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import NO_TS2, prod_vocab  # noqa: F401  (prod_vocab: fixture)
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_transcribe_options_gpu import EOT, PROMPT, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
NEW = 12
NS_TOK = 899
# (recording, seek, n_frames) of the five windows: non-zero seeks, full / odd / tiny / 2 / 1 frames
CUTS = [(0, 1234, 3000), (0, 4000, 1499), (1, 17, 777), (1, 1000, 2), (0, 5000, 1)]
IDS = np.array([(3 << 16) | 17, 5, 1 << 16, 0xFFFF, 9], dtype=np.uint32)


class Five:
    """The five windows on the device, their set on `ctx`, and the arguments of the mel calls on the same windows."""

    def __init__(self, ctx, b):
        self.ctx, self.b = ctx, b
        recs = [np.concatenate([tones(1, 0)[0], tones(1, 2)[0]]), tones(1, 3)[0][:300000]]
        self.mels = ctx.logmel_long(recs)
        self.flat = np.concatenate([m.reshape(-1) for m in self.mels])
        starts = np.cumsum([0] + [m.size for m in self.mels[:-1]]).astype(np.int64)
        self.base = np.array([starts[r] for r, _, _ in CUTS], dtype=np.int64)
        self.T = np.array([self.mels[r].shape[1] for r, _, _ in CUTS], dtype=np.int32)
        self.seek = np.array([s for _, s, _ in CUTS], dtype=np.int32)
        self.nf = np.array([n for _, _, n in CUTS], dtype=np.int32)
        self.d_mel = ctx.to_device(self.flat)
        self.set = ctx.encode_windows(self.d_mel, self.base, self.T, self.seek, self.nf, mem=b.WM_MEM_DEVICE)

    def mel_args(self, rows=None):
        r = np.arange(5) if rows is None else np.asarray(rows)
        return self.d_mel, self.base[r], self.T[r], self.seek[r], self.nf[r]

    def padded(self, rows):
        """the rows' windows zero-padded to 3000 frames (wm_encode's input)"""
        win = np.zeros((len(rows), 80, 3000), dtype=np.float32)
        for i, w in enumerate(rows):
            r, s, n = CUTS[w]
            win[i, :, :n] = self.mels[r][:, s:s + n]
        return win

    def close(self):
        self.set.close()
        self.ctx.dev_free(self.d_mel)


@pytest.fixture(scope="module")
def five(lively, pkg):
    _, _, _, ctx = lively
    f = Five(ctx, pkg.binding)
    yield f
    f.close()


@contextlib.contextmanager
def rules(ctx):
    _rules(ctx)
    try:
        yield
    finally:
        _rules(ctx, False)


def _opts(b, T):
    return b.wm_decode_opts(T, 77, NS_TOK, 0)


def _mel_plain(five, T, rows=None, ids=IDS, new=NEW):
    """wm_transcribe_mel on the windows: (tokens, lens, logprobs, no_speech_prob)"""
    r = np.arange(5) if rows is None else np.asarray(rows)
    return five.ctx.transcribe_mel_raw(*five.mel_args(rows), PROMPT, new, EOT, _opts(five.b, T),
                                       sample_ids=IDS[:len(r)] if ids is None else ids[r],   # (None: IDS by position in the call)
                                       logprobs=True, no_speech=True, mem=five.b.WM_MEM_DEVICE)


def _set_plain(five, T, rows=None, ids=IDS, ctx=None, wset=None, new=NEW):
    """wm_transcribe_windows with best_of = 1 and prompt_len NULL, in the same shape"""
    r = np.arange(5) if rows is None else np.asarray(rows)
    g = (ctx or five.ctx).transcribe_windows_best_of(wset or five.set, rows, PROMPT, new, 1, eot=EOT, temperature=T, seed=77,
                                                     no_speech_token=NS_TOK, sample_ids=ids[r])
    assert np.all(g.best == 0)
    return g.tokens[:, 0], g.lens[:, 0], g.logprobs[:, 0], g.no_speech_prob


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------- 1, 2: the plain call
@pytest.mark.parametrize("T", [0.0, 0.7])
def test_all_windows_equal_wm_transcribe_mel(five, T):
    with rules(five.ctx):
        want = _mel_plain(five, T)
        _same(_set_plain(five, T), want)
    assert len({tuple(t) for t in want[0]}) > 1          # the windows do decode to different tokens


@pytest.mark.parametrize("T", [0.0, 0.7])
def test_rows_in_any_order_with_repeats(five, T):
    rows = [3, 0, 3, 1]
    with rules(five.ctx):
        _same(_set_plain(five, T, rows), _mel_plain(five, T, rows))


# ---------------------------------------------------------------- 3: ragged prompts, best-of, beam
RAGGED = [[7, 8, 9, 10, 21, 5], [10, 21, 5], [3, 10, 22, 5], [1, 2, 3, 4, 5, 6, 10, 23, 5], [10, 24, 5]]


def test_ragged_prompts_equal_wm_transcribe_mel_ragged(five):
    ctx, b = five.ctx, five.b
    with rules(ctx):
        want = ctx.transcribe_mel_raw(*five.mel_args(), RAGGED, NEW, EOT, _opts(b, 0.7), sample_ids=IDS, logprobs=True,
                                      no_speech=True, mem=b.WM_MEM_DEVICE, sot_tail=3)
        g = ctx.transcribe_windows_best_of(five.set, None, RAGGED, NEW, 1, eot=EOT, temperature=0.7, seed=77,
                                           no_speech_token=NS_TOK, sample_ids=IDS, sot_tail=3)
        _same((g.tokens[:, 0], g.lens[:, 0], g.logprobs[:, 0], g.no_speech_prob), want)
        # and through the TranscribeResult mirror
        t = ctx.transcribe_windows(five.set, None, RAGGED, NEW, eot=EOT, temperature=0.7, seed=77, no_speech_token=NS_TOK,
                                   sample_ids=IDS, sot_tail=3)
        _same((t.tokens, t.lens, t.logprobs, t.no_speech_prob), want)


@pytest.mark.parametrize("ragged", [False, True])
def test_best_of_three_equals_wm_transcribe_mel_best_of(five, ragged):
    ctx, b = five.ctx, five.b
    prompts = RAGGED if ragged else PROMPT
    kw = dict(eot=EOT, temperature=0.8, seed=5, no_speech_token=NS_TOK, sample_ids=IDS, length_penalty=0.6)
    if ragged:
        kw["sot_tail"] = 3
    with rules(ctx):
        want = ctx.transcribe_mel_best_of(*five.mel_args(), prompts, NEW, 3, mem=b.WM_MEM_DEVICE, **kw)
        got = ctx.transcribe_windows_best_of(five.set, None, prompts, NEW, 3, **kw)
    _same((got.tokens, got.lens, got.logprobs, got.no_speech_prob, got.best),
          (want.tokens, want.lens, want.logprobs, want.no_speech_prob, want.best))
    assert any(len({tuple(c) for c in w}) > 1 for w in want.tokens)      # candidates that differ


def test_beam_search_equals_wm_transcribe_mel_beam(five):
    ctx, b = five.ctx, five.b
    kw = dict(eot=EOT, no_speech_token=NS_TOK, sot_tail=3, max_candidates=4, length_penalty=None)
    with rules(ctx):
        want = ctx.transcribe_mel_beam(*five.mel_args(), RAGGED, NEW, 3, mem=b.WM_MEM_DEVICE, **kw)
        got = ctx.transcribe_windows_beam(five.set, None, RAGGED, NEW, 3, **kw)
        rows = [4, 2, 2]
        want_r = ctx.transcribe_mel_beam(*five.mel_args(rows), [RAGGED[r] for r in rows], NEW, 3, mem=b.WM_MEM_DEVICE, **kw)
        got_r = ctx.transcribe_windows_beam(five.set, rows, [RAGGED[r] for r in rows], NEW, 3, **kw)
    for g, w in ((got, want), (got_r, want_r)):
        _same((g.tokens, g.lens, g.n_hyp, g.sum_logprob, g.logprobs, g.no_speech_prob, g.best),
              (w.tokens, w.lens, w.n_hyp, w.sum_logprob, w.logprobs, w.no_speech_prob, w.best))


# ---------------------------------------------------------------- 4: groups and lanes
def test_130_rows_span_groups_and_lanes(five):
    ctx = five.ctx
    rows = np.random.default_rng(130).integers(0, 5, size=130)
    ids = np.arange(130, dtype=np.uint32) * 7 + 1
    r = np.arange(130)
    with rules(ctx):
        want = ctx.transcribe_mel_raw(*five.mel_args(rows), PROMPT, 8, EOT, _opts(five.b, 0.7), sample_ids=ids, logprobs=True,
                                      no_speech=True, mem=five.b.WM_MEM_DEVICE)

        def from_set():
            g = ctx.transcribe_windows_best_of(five.set, rows, PROMPT, 8, 1, eot=EOT, temperature=0.7, seed=77,
                                               no_speech_token=NS_TOK, sample_ids=ids[r])
            return g.tokens[:, 0], g.lens[:, 0], g.logprobs[:, 0], g.no_speech_prob
        default = from_set()
        try:
            ctx.set_lanes(1)
            one_lane = from_set()
        finally:
            ctx.set_lanes(0)
    _same(default, want)
    _same(one_lane, want)
    _same(default, one_lane)


def test_a_set_from_host_memory_and_a_set_of_more_than_one_encode_group(five):
    """WM_MEM_HOST copies only the windows; 130 windows are encoded in two groups (128 + 2), whose rows land behind one
    another in the store."""
    ctx, b = five.ctx, five.b
    with rules(ctx):
        want = _mel_plain(five, 0.7)
        with ctx.encode_windows(five.flat, five.base, five.T, five.seek, five.nf) as host:
            _same(_set_plain(five, 0.7, wset=host), want)
        pick = np.random.default_rng(9).integers(0, 5, size=130)
        pick[[0, 127, 128, 129]] = [4, 0, 2, 1]
        with ctx.encode_windows(five.d_mel, five.base[pick], five.T[pick], five.seek[pick], five.nf[pick],
                                mem=b.WM_MEM_DEVICE) as big:
            assert len(big) == 130 and np.array_equal(big.n_frames, five.nf[pick])
            rows = [129, 0, 128, 127, 64]
            g = ctx.transcribe_windows_best_of(big, rows, PROMPT, NEW, 1, eot=EOT, temperature=0.7, seed=77,
                                               no_speech_token=NS_TOK, sample_ids=IDS)
            _same((g.tokens[:, 0], g.lens[:, 0], g.logprobs[:, 0], g.no_speech_prob), _mel_plain(five, 0.7, pick[rows], ids=None))


# ---------------------------------------------------------------- 5: alignment
def test_align_windows_equals_wm_align_mel(five):
    ctx, b = five.ctx, five.b
    rng = np.random.default_rng(5)
    rows = [2, 0, 1, 3, 2]
    texts = [_text(rng, n) for n in (9, 12, 0, 3, 5)]
    sots = [[10, 21 + i, 5] for i in range(5)]
    want = ctx.align_mel(*five.mel_args(rows), texts, sots, NO_TS, EOT, mem=b.WM_MEM_DEVICE)
    got = ctx.align_windows(five.set, rows, texts, sots, NO_TS, EOT)
    _same(got, want)
    assert np.all(got[0][2] == -1) and got[0][0][0] >= 0
    with pytest.raises(b.WhisperError) as e:          # the 1-frame window has no audio frame to align to
        ctx.align_windows(five.set, [0, 4], texts[:2], sots[:2], NO_TS, EOT)
    assert e.value.status == WM_ERR_INVALID and "n_frames" in str(e.value)


# ---------------------------------------------------------------- 6: language identification
@pytest.mark.parametrize("rows", [[2], [4, 0, 1]])
def test_detect_language_equals_encode_then_detect(five, rows):
    ctx = five.ctx
    sot, first, last = 10, 100, 198
    want = ctx.detect_language_probs(ctx.encode_mel(five.padded(rows)), sot, first, last)
    got = ctx.windows_detect_language(five.set, rows, sot, first, last)
    _same(got, want)
    idx = np.empty(len(rows), np.int32)
    r = np.asarray(rows, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert ctx.lib.wm_windows_detect_language(ctx.handle, five.set.handle, p(r), len(rows), sot, first, last, p(idx), None) == 0
    assert np.array_equal(idx, want[0])               # probs NULL: wm_detect_language


# ---------------------------------------------------------------- 7, 10, 11: the set survives, stages, greedy untouched
def test_the_set_survives_other_work_and_greedy_is_unchanged_around_it(lively, five, pkg):
    _, _, _, ctx = lively
    b = pkg.binding
    pcm = tones(9)
    t0, l0 = ctx.transcribe_greedy(pcm[:3], PROMPT, 20, eot=EOT)
    with rules(ctx):
        want = _mel_plain(five, 0.7)
    own = ctx.encode_windows(*five.mel_args(), mem=b.WM_MEM_DEVICE)
    try:
        ms = ctx.last_stage_ms()
        assert ms[1] > 0 and ms[2] == 0                # encoder + cross-K/V + the copy into the store; no decode
        ctx.transcribe_greedy(pcm, PROMPT, 20, eot=EOT)               # other audio, more rows: the lane's caches are reallocated
        mel = ctx.logmel(pcm[:7], out_dtype=np.float32)
        ctx.transcribe_mel_best_of(mel, np.arange(7, dtype=np.int64) * 240000, 3000, 0, 3000, PROMPT, 6, 2, eot=EOT,
                                   temperature=0.5, seed=1)
        with rules(ctx):
            _same(_set_plain(five, 0.7, wset=own), want)
            ms = ctx.last_stage_ms()
            assert ms[0] > 0 and ms[1] == 0 and ms[2] > 0   # the gather, no encoder stage, the decode loop
        rng = np.random.default_rng(6)
        ctx.align_windows(own, [0, 1], [_text(rng, 4), _text(rng, 6)], [10, 21, 5], NO_TS, EOT)
        ctx.windows_detect_language(own, [1, 2], 10, 100, 198)
        ms = ctx.last_stage_ms()
        assert ms[0] > 0 and ms[1] == 0 and ms[2] > 0
    finally:
        own.close()
    t1, l1 = ctx.transcribe_greedy(pcm[:3], PROMPT, 20, eot=EOT)
    assert np.array_equal(t0, t1) and np.array_equal(l0, l1)


# ---------------------------------------------------------------- 8: clones and strangers
def test_a_clone_reads_the_set_and_another_model_does_not(lively, five, pkg):
    dims, _, _, ctx = lively
    b = pkg.binding
    with rules(ctx):
        want = _mel_plain(five, 0.7)
        clone = ctx.clone()                 # (inherits the suppress lists and timestamp rules in force)
        try:
            _same(_set_plain(five, 0.7, ctx=clone), want)
            made_by_clone = clone.encode_windows(*five.mel_args(), mem=b.WM_MEM_DEVICE)
            try:
                _same(_set_plain(five, 0.7, wset=made_by_clone), want)      # ... and the parent reads the clone's
            finally:
                made_by_clone.close()
        finally:
            clone.close()
    for other_dims, seed in ((dims, 4), (dict(dims, n_text_ctx=dims["n_text_ctx"] // 2), 4)):
        other = b.Context(other_dims)
        try:
            other.init_synthetic(seed)
            other.finalize()
            with pytest.raises(b.WhisperError) as e:
                other.transcribe_windows(five.set, None, PROMPT, 4, eot=EOT)
            assert e.value.status == WM_ERR_INVALID and "another model" in str(e.value)
            with pytest.raises(b.WhisperError) as e:
                other.windows_detect_language(five.set, [0], 10, 100, 198)
            assert e.value.status == WM_ERR_INVALID
        finally:
            other.close()


# ---------------------------------------------------------------- 9: arguments
def test_invalid_arguments_and_the_size_formula(lively, five, pkg):
    dims, _, _, ctx = lively
    b, lib = pkg.binding, pkg.binding.load_library()
    assert len(five.set) == 5
    assert five.set.nbytes == 5 * dims["n_text_layer"] * 2 * 1500 * dims["n_text_state"] * 2
    assert np.array_equal(five.set.n_frames, five.nf)
    lib.wm_windows_free(None)
    assert lib.wm_windows_count(None) == -1

    def invalid(fn, *a, **kw):
        with pytest.raises(b.WhisperError) as e:
            fn(*a, **kw)
        assert e.value.status == WM_ERR_INVALID and len(str(e.value)) > 20, str(e.value)

    for rows in ([5], [-1], [0, 1, 7]):                                    # a row outside [0, W)
        invalid(ctx.transcribe_windows, five.set, rows, PROMPT, 4, eot=EOT)
        invalid(ctx.transcribe_windows, five.set, rows, PROMPT, 4, eot=EOT, beam_size=2)
        invalid(ctx.align_windows, five.set, rows, [[1]] * len(rows), PROMPT, NO_TS, EOT)
        invalid(ctx.windows_detect_language, five.set, rows, 10, 100, 198)
    # rows NULL needs B == W; a null set; what the mel counterparts reject
    toks, lens = np.zeros((8, 4), np.int32), np.zeros(8, np.int32)
    pr = np.array(PROMPT, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nan = float("nan")
    call = lambda w, B, best_of=1, stride=0: lib.wm_transcribe_windows(ctx.handle, w, None, B, p(pr), stride, None, 1, None,
                                                                       best_of, nan, 4, EOT, None, p(toks), p(lens), None,
                                                                       None, None)
    assert call(five.set.handle, 3, stride=3) == WM_ERR_INVALID and b"rows is NULL" in lib.wm_last_error()
    assert call(None, 5, stride=3) == WM_ERR_INVALID and b"null window set" in lib.wm_last_error()
    assert call(five.set.handle, 5, stride=0) == WM_ERR_INVALID           # prompt_stride < 1
    assert call(five.set.handle, 5, best_of=9, stride=3) == WM_ERR_INVALID
    assert call(five.set.handle, 0, stride=3) == WM_ERR_INVALID
    invalid(ctx.transcribe_windows, five.set, None, [1, 2, 1 << 20], 4, eot=EOT)       # a token outside the vocabulary
    invalid(ctx.transcribe_windows, five.set, None, PROMPT, 4, eot=EOT, temperature=-1.0)
    invalid(ctx.transcribe_windows, five.set, None, PROMPT, 4, eot=EOT, budgets=[1, 2])   # budgets of another call size
    invalid(ctx.align_windows, five.set, [0], [[EOT + 1]], PROMPT, NO_TS, EOT)          # not a text token
    invalid(ctx.windows_detect_language, five.set, [0], 10, 100, 1 << 20)          # ids outside the vocabulary
    invalid(ctx.encode_windows, five.d_mel, five.base, five.T, five.seek + 100000, five.nf, mem=b.WM_MEM_DEVICE)
    # the all-f32 precision path of the debug library does not support sets
    dbg = b.Context(dims, debug=True)
    try:
        dbg.init_synthetic(1)
        dbg.finalize()
        dbg.set_precision(True)
        with pytest.raises(b.WhisperError) as e:
            dbg.encode_windows(five.flat, five.base, five.T, five.seek, five.nf)
        assert e.value.status == WM_ERR_STATE
    finally:
        dbg.close()


# ---------------------------------------------------------------- 12: transcribe_long
def test_transcribe_long_reuse_encoder_with_fallback_and_best_of(prod):
    recs = _long_recs()
    kw = _kw(best_of=2, logprob_threshold=0.0)           # default temperatures; every window takes all of them
    off = prod.transcribe_long(recs, recording_ids=[7, 300, 65535, 0], **kw)
    on = prod.transcribe_long(recs, recording_ids=[7, 300, 65535, 0], reuse_encoder=True, **kw)
    assert on == off
    assert any(t > 0 for o in off for w in o["windows"] for t in w["temperatures"])
    assert any(w.get("candidate", 0) > 0 for o in off for w in o["windows"])


def test_transcribe_long_reuse_encoder_with_beam_conditioning_words_and_detected_language(prod, prod_vocab):
    recs = _long_recs()
    kw = _kw(beam_size=2, condition_on_previous_text=True, sot_prev=SOT_PREV, vocab=prod_vocab, word_timestamps=True,
             no_timestamps=NO_TS2, language=None)
    off = prod.transcribe_long(recs, **kw)
    on = prod.transcribe_long(recs, reuse_encoder=True, **kw)
    assert on == off
    assert any(s.get("words") for o in off for s in o["segments"])
    assert all(50259 <= o["language"] <= 50357 for o in off)
