"""GPU tests of long-form transcription: wm_logmel_long (openai-whisper's whole-recording log-mel, csrc/frontend.hip),
wm_transcribe_mel (decode from mel windows with per-row prompts and sample ids) and binding.transcribe_long (openai-whisper
transcribe()'s seek loop, batched across recordings).  The numpy restatements are in tests/test_longform_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import whisper_ref as R
from test_longform_cpu import long_log_mel_np, loud_start
from test_model_gpu import _lively_on_device, _perturb_ln_on_device, lively, tones  # noqa: F401  (lively: fixture)
from test_transcribe_options_gpu import EOT, PROMPT, TS, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1   # include/whisper_mi355x.h

LENGTHS = (0, 1, 4000, 480000, 480001, 2_500_123)


def _as(x, dtype):
    if dtype == np.int16:
        return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x.astype(dtype)


def _scaled(x):
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


@pytest.fixture(scope="module")
def fe(pkg):
    ctx = pkg.binding.Context()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_logmel_long_against_the_f64_restatement(fe, pkg, dtype):
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    recs = [_as(0.3 * np.sin(np.arange(n) * 0.013) * (1 + np.cos(np.arange(n) * 1e-4)) if n else np.zeros(0), dtype)
            for n in LENGTHS]
    got = fe.logmel_long(recs)
    ptr, offs, T = fe.logmel_long(recs, device=True)
    try:
        dev = fe.download(ptr, (int(offs[-1]),), np.float32)
    finally:
        fe.dev_free(ptr)
    for r, x in enumerate(recs):
        want = long_log_mel_np(_scaled(x), m80)
        assert got[r].shape == want.shape == (80, (x.size + 480000) // 160)
        err = float(np.abs(got[r] - want).max())
        assert err <= 1e-4, "recording %d (%d samples, %s): max|err| %g" % (r, x.size, np.dtype(dtype).name, err)
        assert np.array_equal(dev[offs[r]:offs[r + 1]].reshape(80, T[r]), got[r])


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_logmel_long_30s_frames_are_bit_identical_to_wm_logmel(fe, dtype):
    x = _as(loud_start(480000, seed=3).astype(np.float64), dtype)
    short = fe.logmel(x[None, :], out_dtype=np.float32)[0]
    assert np.argmax(short.max(axis=0)) < 2999
    long_ = fe.logmel_long([x])[0]
    assert np.array_equal(long_[:, :2999], short[:, :2999])


def test_logmel_long_batch_equals_alone_and_128_mels(fe):
    rng = np.random.default_rng(4)
    recs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (123457, 0, 480000, 700001)]
    both = fe.logmel_long(recs)
    for r, x in enumerate(recs):
        assert np.array_equal(fe.logmel_long([x])[0], both[r])
    # a recording at an odd offset inside a bigger buffer takes the gather path: same bits
    pad = [np.zeros(3, np.float32)] + recs
    assert all(np.array_equal(a, b) for a, b in zip(fe.logmel_long(pad)[1:], both))
    m128 = fe.logmel_long(recs[:1], n_mels=128)[0]
    assert m128.shape == (128, (123457 + 480000) // 160) and np.isfinite(m128).all()


def test_logmel_long_writes_exactly_its_extent(fe, pkg):
    """Canary words before and after the output on the device survive the call."""
    b = pkg.binding
    x = (0.1 * np.random.default_rng(5).standard_normal(4000 + 480001)).astype(np.float32)
    offs = np.array([0, 4000, 4000 + 480001], dtype=np.int64)
    n_out = 80 * ((4000 + 480000) // 160 + (480001 + 480000) // 160)
    CAN = 4096
    d_pcm = fe.to_device(x)
    buf = np.full(n_out + 2 * CAN, 12345.0, dtype=np.float32)
    d_out = fe.to_device(buf)
    try:
        st = fe.lib.wm_logmel_long(fe.handle, d_pcm, b.WM_F32, b._ptr(offs), 2, 80,
                                   ctypes.c_void_p(d_out.value + 4 * CAN), b.WM_MEM_DEVICE)
        assert st == b.WM_OK
        fe.sync()
        got = fe.download(d_out, buf.shape, np.float32)
    finally:
        fe.dev_free(d_pcm)
        fe.dev_free(d_out)
    assert np.all(got[:CAN] == 12345.0) and np.all(got[CAN + n_out:] == 12345.0)
    assert not np.any(got[CAN:CAN + n_out] == 12345.0)


def test_logmel_long_rejects_bad_offsets(fe, pkg):
    b = pkg.binding
    x = np.zeros(10, np.float32)
    out = np.zeros(80 * 3100, np.float32)
    for offs in ([0, 5, 3], [-1, 4]):
        o = np.array(offs, dtype=np.int64)
        assert fe.lib.wm_logmel_long(fe.handle, b._ptr(x), b.WM_F32, b._ptr(o), len(offs) - 1, 80, b._ptr(out),
                                     b.WM_MEM_HOST) == WM_ERR_INVALID
    o = np.array([0, 10], dtype=np.int64)
    assert fe.lib.wm_logmel_long(fe.handle, b._ptr(x), b.WM_F32, b._ptr(o), 1, 64, b._ptr(out),
                                 b.WM_MEM_HOST) == WM_ERR_INVALID


# ---------------------------------------------------------------- wm_transcribe_mel
NEW = 40


def _same(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert np.array_equal(x, y)


@pytest.mark.parametrize("T", [0.0, 0.7])
def test_transcribe_mel_full_windows_equal_wm_transcribe(lively, pkg, T):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    pcm = tones(6)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    opts = b.wm_decode_opts(T, 77, 899, 0)
    want = ctx.transcribe_raw(pcm, PROMPT, NEW, EOT, opts, logprobs=True, no_speech=True)
    base = np.arange(6, dtype=np.int64) * 80 * 3000
    got = ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, PROMPT, NEW, EOT, opts, logprobs=True, no_speech=True)
    _same(got, want)
    d = ctx.to_device(mel)
    try:
        got_d = ctx.transcribe_mel_raw(d, base, 3000, 0, 3000, PROMPT, NEW, EOT, opts, logprobs=True, no_speech=True,
                                       mem=b.WM_MEM_DEVICE)
    finally:
        ctx.dev_free(d)
    _same(got_d, want)
    _rules(ctx, False)


def test_transcribe_mel_window_equals_the_materialised_window(lively, pkg):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    rng = np.random.default_rng(8)
    recs = [tones(1, i)[0][: 480000 - 70000 * i] for i in range(3)] + [np.concatenate([tones(1, 5)[0]] * 2)]
    mels = ctx.logmel_long(recs)
    flat = np.concatenate([m.reshape(-1) for m in mels])
    base = np.cumsum([0] + [m.size for m in mels[:-1]]).astype(np.int64)
    Ts = np.array([m.shape[1] for m in mels], dtype=np.int32)
    content = Ts - 3000
    seek = np.array([rng.integers(0, max(int(c), 1)) for c in content], dtype=np.int32)
    nf = np.array([min(3000, int(c) - int(s)) if c > s else 1 for c, s in zip(content, seek)], dtype=np.int32)
    opts = b.wm_decode_opts(0.0, 0, 899, 0)
    got = ctx.transcribe_mel_raw(flat, base, Ts, seek, nf, PROMPT, NEW, EOT, opts, no_speech=True)
    win = np.zeros((4, 80, 3000), dtype=np.float32)
    for r in range(4):
        win[r, :, :nf[r]] = mels[r][:, seek[r]:seek[r] + nf[r]]
    want = ctx.transcribe_mel_raw(win, np.arange(4, dtype=np.int64) * 240000, 3000, 0, 3000, PROMPT, NEW, EOT, opts,
                                  no_speech=True)
    _same(got, want)
    # and the same windows from device memory
    d = ctx.to_device(flat)
    try:
        _same(ctx.transcribe_mel_raw(d, base, Ts, seek, nf, PROMPT, NEW, EOT, opts, no_speech=True, mem=b.WM_MEM_DEVICE),
              want)
    finally:
        ctx.dev_free(d)
    _rules(ctx, False)


@pytest.mark.parametrize("T", [0.0, 0.9])
def test_per_row_prompts_and_sample_ids_equal_each_row_alone(lively, pkg, T):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    pcm = tones(5)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    base = np.arange(5, dtype=np.int64) * 240000
    prompts = np.array([[10 + r, 21, 5 + r] for r in range(5)], dtype=np.int32)
    ids = np.array([(3 << 16) | 17, 5, 1 << 16, 0xFFFF, 9], dtype=np.uint32)
    opts = b.wm_decode_opts(T, 1234, 899, 0)
    got = ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, prompts, NEW, EOT, opts, sample_ids=ids, no_speech=True)
    for r in range(5):
        one = ctx.transcribe_mel_raw(mel, base[r:r + 1], 3000, 0, 3000, prompts[r:r + 1], NEW, EOT, opts,
                                     sample_ids=ids[r:r + 1], no_speech=True)
        _same([x[r:r + 1] for x in got], one)
    # every prompt equal, ids NULL: wm_transcribe
    want = ctx.transcribe_raw(pcm, PROMPT, NEW, EOT, opts, no_speech=True)
    same = np.tile(np.array(PROMPT, dtype=np.int32), (5, 1))
    _same(ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, same, NEW, EOT, opts, no_speech=True), want)
    if T > 0:
        # ids = the call indices 0 .. 4 are the NULL counter; other ids give other samples
        _same(ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, same, NEW, EOT, opts, no_speech=True,
                                     sample_ids=np.arange(5, dtype=np.uint32)), want)
        other = ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, same, NEW, EOT, opts, no_speech=True,
                                       sample_ids=np.arange(5, dtype=np.uint32) + 1000)
        assert not np.array_equal(other[0], want[0])
    _rules(ctx, False)


def test_sample_ids_select_the_philox_counter(lively, pkg):
    """A row sampled with id k is the row with call index k: decode 7 rows (ids NULL), then row 6's window alone with
    sample id 6 and any other row's prompt equal: same tokens."""
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    pcm = tones(7)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    opts = b.wm_decode_opts(1.0, 99, 899, 0)
    want = ctx.transcribe_raw(pcm, PROMPT, NEW, EOT, opts)
    for r in (0, 6):
        one = ctx.transcribe_mel_raw(mel, np.array([r * 240000], np.int64), 3000, 0, 3000, PROMPT, NEW, EOT, opts,
                                     sample_ids=np.array([r], np.uint32))
        assert np.array_equal(one[0][0], want[0][r]) and np.array_equal(one[2][0], want[2][r])
    _rules(ctx, False)


def test_transcribe_mel_rejects_invalid_windows_and_prompts(lively, pkg):
    _, _, _, ctx = lively
    b = pkg.binding
    mel = np.zeros((1, 80, 3000), np.float32)
    bad = [dict(seek=-1), dict(n_frames=0), dict(n_frames=3001), dict(seek=1), dict(mel_len=0), dict(base=-5)]
    for kw in bad:
        with pytest.raises(b.WhisperError) as e:
            ctx.transcribe_mel_raw(mel, np.array([kw.get("base", 0)], np.int64), kw.get("mel_len", 3000),
                                   kw.get("seek", 0), kw.get("n_frames", 3000), PROMPT, 4, EOT)
        assert e.value.status == WM_ERR_INVALID
    with pytest.raises(b.WhisperError) as e:
        ctx.transcribe_mel_raw(np.zeros((2, 80, 3000), np.float32), np.array([0, 240000], np.int64), 3000, 0, 3000,
                               np.array([[1, 2, 3], [1, 2, 1 << 20]], np.int32), 4, EOT)
    assert e.value.status == WM_ERR_INVALID


# ---------------------------------------------------------------- transcribe_long
SOT, TASK, SOT_PREV, NS, TSB, EOT2 = 50258, 50359, 50361, 50362, 50364, 50257


@pytest.fixture(scope="module")
def prod(pkg):
    """The lively tiny model with the production vocabulary (real timestamp ids) and a short text context."""
    dims = dict(R.TINY_DIMS, n_vocab=51865, n_text_ctx=64)
    ctx = pkg.binding.Context(dims)
    ctx.init_synthetic(29)
    _perturb_ln_on_device(ctx, dims, seed=6)
    _lively_on_device(ctx, dims)
    ctx.finalize()
    ctx.set_suppress([SOT, SOT_PREV, NS, 50363, 50358], [220, EOT2])
    yield ctx
    ctx.close()


def _long_recs():
    n = np.arange(95 * 16000, dtype=np.float64)
    tone = (0.3 * np.sin(2 * np.pi * 310 * n / 16000) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.37 * n / 16000))).astype(
        np.float32)
    return [tone[:12 * 16000 + 123], tone[5000:5000 + 45 * 16000], tone, np.zeros(20 * 16000, np.float32)]


def _kw(**extra):
    kw = dict(sot=SOT, task=TASK, eot=EOT2, timestamp_begin=TSB, no_speech_token=NS, lang_first=50259,
              lang_last=50357)
    kw.update(extra)
    return kw


def _strip(o):
    return (o["language"], o["seeks"], [(w["seek"], w["segment_size"], w["temperatures"], w["skipped"], w["tokens"])
                                        for w in o["windows"]], o["segments"])


@pytest.mark.parametrize("forced", [False, True])
def test_transcribe_long_batched_equals_each_recording_alone(prod, forced):
    recs = _long_recs()
    kw = _kw(logprob_threshold=0.0) if forced else _kw()
    ids = [7, 300, 65535, 0]
    got = prod.transcribe_long(recs, recording_ids=ids, **kw)
    if forced:   # every window fell back: sampled windows are covered
        assert any(t > 0 for o in got for w in o["windows"] for t in w["temperatures"])
    for r, x in enumerate(recs):
        alone = prod.transcribe_long([x], recording_ids=[ids[r]], **kw)[0]
        assert _strip(alone) == _strip(got[r]), "recording %d" % r
    for o, x in zip(got, recs):
        content = (x.size + 480000) // 160 - 3000
        assert o["seeks"] == sorted(o["seeks"]) and all(s < content for s in o["seeks"])
        last_end = 0.0
        for s in o["segments"]:
            if not s["tokens"]:
                continue
            assert s["start"] >= last_end - 1e-9 and s["start"] <= s["end"]
            # within the window that produced it (openai-whisper does not clip a timestamp of the zero-padded tail to
            # the recording's duration, and neither do these rules: the random model's timestamps can lie there)
            assert s["seek"] * 0.01 <= s["start"] and s["end"] <= s["seek"] * 0.01 + 30.0 + 1e-9
            assert s["seek"] < content
            last_end = s["end"]
    # the silent recording: one window per 30 s of content at most -- a window's seek never goes backwards
    assert len(got[3]["windows"]) >= 1 and got[3]["seeks"][0] == 0


def test_transcribe_long_given_language_and_initial_prompt(prod):
    recs = _long_recs()[:2]
    out = prod.transcribe_long(recs, language=[50259, 50260], sot_prev=SOT_PREV, initial_prompt_tokens=[400, 401, 402],
                               **_kw())
    assert [o["language"] for o in out] == [50259, 50260]
    for o, x in zip(out, recs):
        content = (x.size + 480000) // 160 - 3000
        assert o["seeks"][0] == 0
        assert all(w["segment_size"] == min(3000, content - w["seek"]) for w in o["windows"])
    detected = prod.transcribe_long(recs[:1], **_kw())[0]["language"]
    assert 50259 <= detected <= 50357
