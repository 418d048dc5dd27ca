"""CPU tests of the input side for audio at any sample rate: the resampler's filter and length rule (wm_resample_filter,
wm_resample_out_len: host only), the general RIFF/WAVE reader (wm_audio_*, csrc/audio.cpp) and the sample_rates plumbing of
binding.transcribe_long on a stub context.  The f64 restatement is tests/resample_ref.py; the kernel's own tests are in
tests/test_resample_gpu.py."""
import ctypes
import importlib
import os
import struct
import wave

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import resample_ref as ref

B = importlib.import_module("openai_whisper_coreml_amd.binding")

FUZZ = settings(max_examples=int(os.environ.get("WM_FUZZ_EXAMPLES", "120")), deadline=None,
                suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.binding.load_library()


# ---------------------------------------------------------------- the filter
@pytest.mark.parametrize("sr", ref.RATES)
def test_filter_table_matches_the_f64_restatement(lib, sr):
    h64, L, M, K = ref.prototype(sr)
    h, l, m, k = B.resample_filter(sr)
    assert (l, m, k) == (L, M, K) and h.dtype == np.float32 and h.size == 2 * K + 1
    err = np.abs(h.astype(np.float64) - h64).max()
    print("rate %d: L %d M %d K %d, max |h_f32 - h_f64| = %.3e (gate %.3e)" % (sr, L, M, K, err, 2.0 ** -23 * np.abs(h64).max()))
    assert err <= 2.0 ** -23 * np.abs(h64).max()
    assert np.array_equal(h.view(np.uint32), h[::-1].view(np.uint32))     # symmetric bit for bit
    # the window is numpy's Kaiser window, the restatement's I0 series against numpy's own i0
    j = np.arange(-K, K + 1)
    c = 0.9 / (2 * max(L, M))
    assert np.abs(L * 2 * c * np.sinc(2 * c * j) * np.kaiser(2 * K + 1, 9.62) - h64).max() <= 1e-12 * np.abs(h64).max()


def test_filter_sizing_call_and_rejections(lib):
    L, M, K = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.wm_resample_filter(44100, None, 0, ctypes.byref(L), ctypes.byref(M), ctypes.byref(K)) == 0
    assert (L.value, M.value, K.value) == (160, 441, 32 * 441)
    assert -(-(2 * K.value + 1) // L.value) == 177 == ref.taps(44100)
    assert [ref.taps(sr) for sr in (48000, 8000, 11025, 96000)] == [193, 65, 65, 385]
    buf = np.zeros(16, np.float32)
    assert lib.wm_resample_filter(44100, buf.ctypes.data_as(ctypes.c_void_p), 16, None, None, None) == 1   # too small
    assert lib.wm_resample_filter(44100, None, 2 * K.value + 1, None, None, None) == 1                      # null table
    for bad in (44101, 3999, 200000, 0, -48000):
        assert lib.wm_resample_filter(bad, None, 0, None, None, None) == 1, bad      # WM_ERR_INVALID
        assert str(bad).encode() in lib.wm_last_error()
        assert lib.wm_resample_out_len(100, bad) == -1
    assert not ref.supported(44101) and all(ref.supported(sr) for sr in ref.RATES)


def test_out_len(lib):
    for sr in ref.RATES + (5000, 4000):
        L, M, _ = ref.params(sr)
        for n in (0, 1, 2, 440, 441, 442, 10 ** 9):
            assert lib.wm_resample_out_len(n, sr) == -(-n * L // M) == B.resample_out_len(n, sr), (n, sr)
    assert lib.wm_resample_out_len(-1, 48000) == -1
    with pytest.raises(ValueError):
        B.resample_out_len(10, 44101)


@pytest.mark.parametrize("sr", (48000, 44100, 8000, 11025))
def test_restatement_matches_scipy_resample_poly(sr):
    sig = pytest.importorskip("scipy.signal")
    h, L, M, K = ref.prototype(sr)
    rng = np.random.default_rng(sr)
    for n in (1, 2, 700, 1501):
        x = rng.uniform(-1, 1, n)
        want = sig.resample_poly(x, L, M, window=h / L)
        got = ref.resample(x, sr)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13, (sr, n, np.abs(got - want).max())


def test_downmix_restatement():
    x = np.array([[32767, -32768, 1], [3, 4, 5]], dtype=np.int16)
    m = ref.downmix(x)
    f = x.astype(np.float32) / np.float32(32768)
    assert m.dtype == np.float32 and np.array_equal(m, ((f[:, 0] + f[:, 1]) + f[:, 2]) * np.float32(1.0 / 3))
    assert np.array_equal(ref.downmix(x[:, 0]), f[:, 0]) and np.array_equal(ref.downmix(x[:, :1]), f[:, 0])


# ---------------------------------------------------------------- wm_audio_*
def _ints(bits, n, channels, rng):
    lo, hi = (0, 256) if bits == 8 else (-(1 << (bits - 1)), 1 << (bits - 1))
    v = rng.integers(lo, hi, size=(n, channels), dtype=np.int64)
    v.flat[:2] = (lo, hi - 1)
    return v


def _int_bytes(v, bits):
    if bits == 8:
        return v.astype(np.uint8).tobytes()
    if bits == 24:
        b = v.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    return v.astype("<i%d" % (bits // 8)).tobytes()


def _int_expected(v, bits):
    if bits == 8:
        return ((v - 128).astype(np.float32) / np.float32(128))
    if bits == 32:
        return (v.astype(np.float64) / 2147483648.0).astype(np.float32)
    return v.astype(np.float32) / np.float32(1 << (bits - 1))


def _riff(fmt_body, data, data_len=None, extra=b"", pad_byte=b""):
    dl = len(data) if data_len is None else data_len
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body + extra + b"data" + struct.pack("<I", dl & 0xffffffff) + data + pad_byte
    return b"RIFF" + struct.pack("<I", len(body) & 0xffffffff) + body


def _fmt(tag, channels, rate, bits, align=None, extensible_sub=None):
    align = channels * bits // 8 if align is None else align
    head = struct.pack("<HHIIHH", tag, channels, rate, (rate * align) & 0xffffffff, align, bits)
    if extensible_sub is None:
        return head
    guid_tail = bytes.fromhex("000000001000800000aa00389b71")
    return head + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", extensible_sub) + guid_tail


@pytest.mark.parametrize("bits", (8, 16, 24, 32))
@pytest.mark.parametrize("channels,rate", ((1, 48000), (2, 44100), (3, 8000)))
def test_audio_reads_what_the_wave_module_writes(lib, tmp_path, bits, channels, rate):
    rng = np.random.default_rng(bits * 10 + channels)
    v = _ints(bits, 301, channels, rng)
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(bits // 8)
        w.setframerate(rate)
        w.writeframes(_int_bytes(v, bits))
    a = B.Audio(p)
    assert (a.sample_rate, a.channels, a.num_frames, a.bits, a.is_float) == (rate, channels, 301, bits, False)
    want = _int_expected(v, bits)
    got = a.read()
    assert got.dtype == np.float32 and got.shape == (301, channels) and np.array_equal(got, want)
    assert np.array_equal(a.read(7, 100), want[7:107]) and a.read(301, 0).shape == (0, channels)      # partial reads
    for first, n in ((0, 302), (301, 1), (-1, 1), (5, -1), (2 ** 62, 2 ** 62)):                      # out of range
        with pytest.raises(B.WhisperError) as e:
            a.read(first, n)
        assert e.value.status == 1
    if bits == 16:
        assert np.array_equal(a.read(3, 50, raw_int16=True), v[3:53].astype(np.int16))
    else:
        with pytest.raises(B.WhisperError):
            a.read(0, 1, raw_int16=True)
    a.close()
    # the strict reader keeps its rule
    h = ctypes.c_void_p()
    assert lib.wm_wav_open(p.encode(), ctypes.byref(h)) == 4 and not h.value


def test_audio_float_and_extensible_headers(lib, tmp_path):
    rng = np.random.default_rng(5)
    x32 = rng.uniform(-1, 1, (50, 2)).astype(np.float32)
    x64 = rng.uniform(-1, 1, (50, 2))
    x64[0] = (1e300, -1e300)
    i24 = _ints(24, 50, 2, rng)
    i16 = _ints(16, 50, 1, rng)
    cases = [
        (_fmt(3, 2, 96000, 32), x32.astype("<f4").tobytes(), x32, True, 32),
        (_fmt(3, 2, 22050, 64), x64.astype("<f8").tobytes(), None, True, 64),
        (_fmt(0xFFFE, 2, 48000, 32, extensible_sub=3), x32.astype("<f4").tobytes(), x32, True, 32),
        (_fmt(0xFFFE, 2, 48000, 24, extensible_sub=1), _int_bytes(i24, 24), _int_expected(i24, 24), False, 24),
        (_fmt(0xFFFE, 1, 16000, 16, extensible_sub=1), _int_bytes(i16, 16), _int_expected(i16, 16), False, 16),
    ]
    for k, (fmt_body, data, want, is_float, bits) in enumerate(cases):
        p = tmp_path / ("f%d.wav" % k)
        p.write_bytes(_riff(fmt_body, data, extra=b"LIST" + struct.pack("<I", 3) + b"abc\0"))       # an odd, padded chunk first
        a = B.Audio(p)
        assert (a.num_frames, a.is_float, a.bits) == (50, is_float, bits)
        got = a.read()
        if want is None:
            with np.errstate(over="ignore"):
                want = x64.astype(np.float32)
            assert np.isinf(got[0]).all()
        assert np.array_equal(got, want), k
        a.close()


def test_audio_truncated_streamed_and_inconsistent_files(lib, tmp_path):
    v = _ints(16, 100, 2, np.random.default_rng(1))
    data = _int_bytes(v, 16)
    want = _int_expected(v, 16)

    def opened(name, blob):
        p = tmp_path / name
        p.write_bytes(blob)
        return B.Audio(p)

    a = opened("trunc.wav", _riff(_fmt(1, 2, 48000, 16), data[:4 * 60 + 3], data_len=len(data)))     # data chunk cut mid-frame
    assert a.num_frames == 60 and np.array_equal(a.read(), want[:60])
    a = opened("stream.wav", _riff(_fmt(1, 2, 48000, 16), data, data_len=0xFFFFFFFF))                # streamed: length unknown
    assert a.num_frames == 100 and np.array_equal(a.read(), want)
    a = opened("empty.wav", _riff(_fmt(1, 2, 48000, 16), b""))
    assert a.num_frames == 0 and a.read().shape == (0, 2)
    bad = {
        "align": _riff(_fmt(1, 2, 48000, 16, align=2), data),
        "bits12": _riff(_fmt(1, 2, 48000, 12, align=4), data),
        "float16": _riff(_fmt(3, 2, 48000, 16), data),
        "ch0": _riff(_fmt(1, 0, 48000, 16, align=2), data),
        "ch9": _riff(_fmt(1, 9, 48000, 16), data),
        "rate0": _riff(_fmt(1, 2, 0, 16), data),
        "adpcm": _riff(_fmt(2, 2, 48000, 16), data),
        "ext_short": _riff(_fmt(0xFFFE, 2, 48000, 16), data),
        "ext_sub": _riff(_fmt(0xFFFE, 2, 48000, 16, extensible_sub=7), data),
        "no_fmt": b"RIFF" + struct.pack("<I", 12 + len(data)) + b"WAVE" + b"data" + struct.pack("<I", len(data)) + data,
        "no_data": _riff(_fmt(1, 2, 48000, 16), b"")[:-8],
        "not_riff": b"RIFX" + _riff(_fmt(1, 2, 48000, 16), data)[4:],
        "short": b"RIFF\0\0",
        "fmt_cut": _riff(_fmt(1, 2, 48000, 16), data)[:30],
    }
    for name, blob in bad.items():
        p = tmp_path / (name + ".wav")
        p.write_bytes(blob)
        h = ctypes.c_void_p()
        assert lib.wm_audio_open(str(p).encode(), ctypes.byref(h)) == 4 and not h.value, name       # WM_ERR_IO
        assert lib.wm_last_error()
    h = ctypes.c_void_p()
    assert lib.wm_audio_open(str(tmp_path / "missing.wav").encode(), ctypes.byref(h)) == 4
    assert lib.wm_audio_open(None, ctypes.byref(h)) == 1
    assert lib.wm_audio_num_frames(None) == 0 and lib.wm_audio_channels(None) == 0 and lib.wm_audio_sample_rate(None) == 0
    assert lib.wm_audio_read(None, 0, 0, None) == 1
    lib.wm_audio_close(None)


def _try_audio(lib, path):
    """Open + read through the C ABI the way a host would: OK or an error, and nothing written outside the buffer."""
    h = ctypes.c_void_p()
    st_ = lib.wm_audio_open(path.encode(), ctypes.byref(h))
    if st_ != 0:
        assert not h.value and lib.wm_last_error()
        return st_
    n, c = lib.wm_audio_num_frames(h), lib.wm_audio_channels(h)
    assert n >= 0 and 1 <= c <= 8 and lib.wm_audio_sample_rate(h) >= 1 and lib.wm_audio_bits(h) in (8, 16, 24, 32, 64)
    take = min(n, 1000)
    guard = 256
    out = np.full(take * c + 2 * guard, 7.5, dtype=np.float32)
    assert lib.wm_audio_read(h, n - take, take, out[guard:].ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.all(out[:guard] == 7.5) and np.all(out[guard + take * c:] == 7.5), "wm_audio_read wrote outside its buffer"
    assert lib.wm_audio_read(h, n, 1, out[guard:].ctypes.data_as(ctypes.c_void_p)) != 0
    assert lib.wm_audio_read(h, -1, 1, out[guard:].ctypes.data_as(ctypes.c_void_p)) != 0
    o16 = np.zeros(take * c + 1, dtype=np.int16)
    lib.wm_audio_read_i16(h, n - take, take, o16.ctypes.data_as(ctypes.c_void_p))
    lib.wm_audio_close(h)
    return 0


@FUZZ
@given(tag=st.sampled_from([0, 1, 2, 3, 0xFFFE, 0xFFFF]), channels=st.integers(0, 10), rate=st.sampled_from([0, 1, 8000, 48000, 2 ** 32 - 1]),
       bits=st.sampled_from([0, 1, 8, 12, 16, 24, 32, 64, 65528]), align=st.one_of(st.none(), st.integers(0, 65535)),
       sub=st.one_of(st.none(), st.sampled_from([0, 1, 3, 9])), n_data=st.integers(0, 600),
       data_len=st.one_of(st.none(), st.integers(0, 2 ** 32 - 1)), cut=st.integers(0, 120), odd=st.booleans())
def test_fuzz_audio_headers(lib, tmp_path, tag, channels, rate, bits, align, sub, n_data, data_len, cut, odd):
    fmt_body = _fmt(tag, channels, rate, bits, align=align if align is not None else (channels * bits // 8) & 0xffff,
                    extensible_sub=sub if tag == 0xFFFE else None)
    extra = (b"junk" + struct.pack("<I", 5) + b"12345" + (b"\0" if not odd else b"")) if odd or cut % 2 else b""
    blob = _riff(fmt_body, bytes(range(256)) * 3 if n_data > 300 else bytes(n_data), data_len=data_len, extra=extra)
    blob = blob[:max(0, len(blob) - cut)]
    p = tmp_path / "fuzz.wav"
    p.write_bytes(blob)
    assert _try_audio(lib, str(p)) in (0, 1, 4)


@FUZZ
@given(flips=st.lists(st.tuples(st.integers(0, 99), st.integers(0, 255)), min_size=1, max_size=6), trunc=st.integers(0, 100))
def test_fuzz_audio_mutated_bytes(lib, tmp_path, flips, trunc):
    blob = bytearray(_riff(_fmt(0xFFFE, 2, 44100, 24, extensible_sub=1), bytes(range(120)),
                           extra=b"LIST" + struct.pack("<I", 3) + b"abc\0"))
    for pos, val in flips:
        blob[pos % len(blob)] = val
    p = tmp_path / "mut.wav"
    p.write_bytes(bytes(blob[:len(blob) - trunc]))
    assert _try_audio(lib, str(p)) in (0, 1, 4)


# ---------------------------------------------------------------- packing and transcribe_long(sample_rates=...) on a stub
def test_pack_interleaved():
    a = np.arange(6, dtype=np.int16).reshape(3, 2)
    b = np.arange(4, dtype=np.int16)
    pcm, offs, ch, sr = B._pack_interleaved([a, b], [48000, 8000])
    assert pcm.dtype == np.int16 and list(pcm) == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3] and list(offs) == [0, 6, 10]
    assert list(ch) == [2, 1] and list(sr) == [48000, 8000] and ch.dtype == sr.dtype == np.int32
    pcm, offs, ch, sr = B._pack_interleaved([a, b.astype(np.float32)], [48000, 8000])
    assert pcm.dtype == np.float32 and np.array_equal(pcm[:6], a.reshape(-1).astype(np.float32) / np.float32(32768))
    with pytest.raises(ValueError):
        B._pack_interleaved([a], [48000, 8000])
    with pytest.raises(ValueError):
        B._pack_interleaved([a.astype(np.float64)], [48000])


SOT, LANG, TASK, SOT_PREV, NS, TSB, EOT = 50258, 50259, 50359, 50361, 50362, 50364, 50257


class StubCtx:
    """Records every context call transcribe_long makes; every window decodes to one 10 s segment."""

    def __init__(self):
        self.dims = dict(n_text_ctx=64, n_mels=80, n_vocab=51865)
        self.calls = []

    def set_timestamp_rules(self, *a):
        self.calls.append(("set_timestamp_rules",))

    def _mel(self, lens, n_mels):
        T = np.array([(n + 480000) // 160 for n in lens], dtype=np.int32)
        return ctypes.c_void_p(4096), np.concatenate([[0], np.cumsum(T.astype(np.int64) * n_mels)]), T

    def logmel_long(self, recordings, n_mels=80, device=False):
        self.calls.append(("logmel_long", [len(r) for r in recordings], device))
        return self._mel([len(r) for r in recordings], n_mels)

    def resample_16k(self, recordings, sample_rates, device=False):
        self.calls.append(("resample_16k", [np.asarray(r).shape for r in recordings], list(sample_rates), device))
        offs = np.concatenate([[0], np.cumsum([ref.out_len(len(r), sr) for r, sr in zip(recordings, sample_rates)])]).astype(np.int64)
        return ctypes.c_void_p(8192), offs

    def logmel_long_device(self, d_pcm, dtype, sample_offsets, n_mels=80):
        self.calls.append(("logmel_long_device", d_pcm.value, np.dtype(dtype), [int(x) for x in sample_offsets]))
        return self._mel(np.diff(sample_offsets), n_mels)

    def dev_free(self, p):
        self.calls.append(("dev_free", p.value))

    def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, eot=-1, temperature=0.0, seed=0,
                       no_speech_token=-1, sot_index=0, sample_ids=None, mem=0, budgets=None, prompt_len=None, sot_tail=None):
        self.calls.append(("transcribe_mel", mel.value, [int(x) for x in mel_len], [int(x) for x in seek], [int(x) for x in n_frames]))
        n = len(sample_ids)
        body = [TSB, 1000, 2000, TSB + 500, TSB + 500, eot]
        toks = np.full((n, max_new), eot, dtype=np.int32)
        toks[:, :len(body)] = body
        lp = np.zeros((n, max_new), dtype=np.float32)
        lp[:, :len(body)] = -0.1
        return B.TranscribeResult(toks, np.full(n, len(body), dtype=np.int32), lp, np.full(n, 0.01, dtype=np.float32), eot)


def _kw():
    return dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, language=LANG, compression_ratio_threshold=None)


def test_transcribe_long_resamples_on_the_device_and_reads_that_buffer():
    recs = [np.zeros((48000 * 12, 2), np.int16), np.zeros(44100 * 25, np.float32)]
    ctx = StubCtx()
    out = B.transcribe_long(ctx, recs, sample_rates=[48000, 44100], **_kw())
    names = [c[0] for c in ctx.calls]
    assert names.count("resample_16k") == 1 and names.count("logmel_long_device") == 1 and "logmel_long" not in names
    rs = ctx.calls[names.index("resample_16k")]
    assert rs[1:] == ([(48000 * 12, 2), (44100 * 25,)], [48000, 44100], True)
    lm = ctx.calls[names.index("logmel_long_device")]
    assert lm[1:] == (8192, np.dtype(np.float32), [0, 16000 * 12, 16000 * 37])       # the resampler's device pointer and offsets
    # the 16 kHz buffer is freed once the log-mel exists, the log-mel at the end; nothing else touches the input
    assert names.index("logmel_long_device") < names.index("dev_free") and ctx.calls[names.index("dev_free")] == ("dev_free", 8192)
    assert ctx.calls[-1] == ("dev_free", 4096)
    # and the rounds behind it are those of the same recordings given at 16 kHz
    ctx16 = StubCtx()
    out16 = B.transcribe_long(ctx16, [np.zeros(16000 * 12, np.float32), np.zeros(16000 * 25, np.float32)], **_kw())
    assert [c for c in ctx.calls if c[0] == "transcribe_mel"] == [c for c in ctx16.calls if c[0] == "transcribe_mel"]
    assert [o["seeks"] for o in out] == [o["seeks"] for o in out16] and [len(o["segments"]) for o in out] == [2, 3]


def test_transcribe_long_without_sample_rates_makes_the_calls_it_made():
    ctx = StubCtx()
    B.transcribe_long(ctx, [np.zeros(16000 * 12, np.float32), np.zeros(16000 * 25, np.float32)], **_kw())
    assert [c[0] for c in ctx.calls] == ["set_timestamp_rules", "logmel_long", "transcribe_mel", "transcribe_mel", "transcribe_mel",
                                         "dev_free"]
    assert ctx.calls[1] == ("logmel_long", [16000 * 12, 16000 * 25], True) and ctx.calls[-1] == ("dev_free", 4096)
    with pytest.raises(ValueError):
        B.transcribe_long(StubCtx(), [np.zeros(100, np.float32)], sample_rates=[48000, 8000], **_kw())
