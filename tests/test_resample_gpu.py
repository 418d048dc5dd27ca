"""GPU tests of wm_resample_16k (csrc/resample.hip): recordings at any rate and channel count -> 16 kHz mono f32, against
the f64 restatement tests/resample_ref.py.

Gate: |y - y_ref| <= (T + 2) * 2^-24 * 2.23 * max|m|, T = taps per output of the rate, 2.23 = the largest per-phase sum of
|h|: the worst case of an f32 sum of T products in any order plus one rounding each of coefficient and sample -- derived,
not measured.  Every comparison prints the maximum it saw."""
import ctypes
import importlib

import numpy as np
import pytest

import resample_ref as ref
from test_model_gpu import _lively_on_device, _perturb_ln_on_device
from oracle import whisper_ref as R

B = importlib.import_module("openai_whisper_coreml_amd.binding")

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1
TILE = 1024   # outputs per workgroup (csrc/resample.hip RS_TILE)
RATES = (48000, 32000, 96000, 44100, 11025, 8000)


@pytest.fixture(scope="module")
def fe(pkg):
    ctx = pkg.binding.Context()
    yield ctx
    ctx.close()


def gate(sr, m):
    return (ref.taps(sr) + 2) * 2.0 ** -24 * 2.23 * (float(np.abs(m).max()) if m.size else 0.0)


def frames_for_outputs(sr, n_out):
    """The fewest input frames that give at least n_out outputs."""
    L, M, _ = ref.params(sr)
    n = n_out * M // L
    while ref.out_len(n, sr) < n_out:
        n += 1
    return n


def lengths(sr):
    L, M, K = ref.params(sr)
    half = -(-K // L)          # the filter's half-width in input frames
    return [0, 1, 2, half - 1] + [frames_for_outputs(sr, t) for t in (TILE - 1, TILE, TILE + 1)] + [5000]


def signal(rng, n, channels, dtype):
    shape = (n,) if channels == 1 else (n, channels)
    if dtype == np.int16:
        x = rng.integers(-32768, 32768, size=shape, dtype=np.int64).astype(np.int16)
        if n:
            x.flat[0] = -32768
            x.flat[-1] = 32767
        return x
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


_REF = {}


def reference(sr, x):
    """(mono f32, y f64) of one recording; the prototype of a rate is built once."""
    if sr not in _REF:
        _REF[sr] = ref.prototype(sr)[0]
    m = ref.downmix(x)
    return m, ref.resample(m, sr, _REF[sr])


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("sr", RATES)
def test_rates_lengths_and_layouts_against_the_f64_restatement(fe, sr, dtype):
    rng = np.random.default_rng(sr + (1 if dtype == np.int16 else 0))
    recs = [signal(rng, n, c, dtype) for n in lengths(sr) for c in (1, 2, 3)]
    got = fe.resample_16k(recs, [sr] * len(recs))
    worst = 0.0
    for x, y in zip(recs, got):
        m, want = reference(sr, x)
        assert y.dtype == np.float32 and y.shape == want.shape == (ref.out_len(len(x), sr),)
        if not y.size:
            continue
        err = float(np.abs(y - want).max())
        worst = max(worst, err / max(float(np.abs(m).max()), 1e-30))
        assert err <= gate(sr, m), "rate %d, %r %s: max|err| %g > gate %g" % (sr, x.shape, x.dtype, err, gate(sr, m))
    print("rate %d %s: taps %d, worst max|err| / max|m| = %.3e (gate %.3e)" % (sr, np.dtype(dtype).name, ref.taps(sr), worst,
                                                                             gate(sr, np.ones(1))))


@pytest.mark.parametrize("sr", RATES)
def test_impulses_give_the_matching_slice_of_the_filter(fe, sr):
    h, L, M, K = B.resample_filter(sr)
    N = 3000
    recs = []
    for k in (0, 1, N - 2, N - 1):
        x = np.zeros(N, np.float32)
        x[k] = 1.0
        recs.append(x)
    got = fe.resample_16k(recs, [sr] * 4)
    n = np.arange(ref.out_len(N, sr), dtype=np.int64)
    for k, y in zip((0, 1, N - 2, N - 1), got):
        j = n * M - k * L
        want = np.where(np.abs(j) <= K, h[np.clip(j + K, 0, 2 * K)], np.float32(0))
        assert np.array_equal(y, want), "rate %d, impulse at %d" % (sr, k)      # one exact product per output
        assert np.count_nonzero(y) > 0


@pytest.mark.parametrize("sr", RATES)
def test_constant_one(fe, sr):
    N = frames_for_outputs(sr, TILE + 300)
    x = np.ones(N, np.float32)
    y = fe.resample_16k([x], [sr])[0]
    m, want = reference(sr, x)
    err = float(np.abs(y - want).max())
    print("rate %d constant: max|err| %.3e (gate %.3e), y[0] %.4f, interior max|y - 1| %.3e" % (
        sr, err, gate(sr, m), y[0], np.abs(y[200:-200] - 1).max()))
    assert err <= gate(sr, m)
    # the restatement's own shape: unit gain inside (DC gain 1.000002, images below -96 dB); at the edge the zero padding
    # takes one side of the filter away: y[0] = h[0] + (1 - h[0]) / 2 with h[0] = 0.9 L / max(L, M)
    L, M, _ = ref.params(sr)
    edge = (1 + 0.9 * L / max(L, M)) / 2
    assert np.abs(want[200:-200] - 1).max() <= 1e-4 and abs(want[0] - edge) <= 1e-4 and abs(want[-1] - 1) > 1e-2
    assert np.abs(y[200:-200] - 1).max() <= 1e-4 + gate(sr, m) and abs(y[0] - edge) <= 1e-4 + gate(sr, m)


def test_16000_hz_is_a_downmix_only(fe):
    rng = np.random.default_rng(16)
    mono = signal(rng, TILE + 77, 1, np.float32)
    st32 = signal(rng, 2500, 2, np.float32)
    tri = signal(rng, 333, 3, np.float32)
    got = fe.resample_16k([mono, st32, tri, np.zeros(0, np.float32)], [16000] * 4)
    assert np.array_equal(got[0].view(np.uint32), mono.view(np.uint32))
    assert np.array_equal(got[1], (st32[:, 0] + st32[:, 1]) * np.float32(0.5))
    assert np.array_equal(got[2], ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * np.float32(1.0 / 3))
    assert got[3].size == 0
    i16 = signal(rng, 4097, 1, np.int16)
    st16 = signal(rng, 1500, 2, np.int16)
    got = fe.resample_16k([i16, st16], [16000, 16000])
    f = st16.astype(np.float32) / np.float32(32768)
    assert np.array_equal(got[0], i16.astype(np.float32) / np.float32(32768))
    assert np.array_equal(got[1], (f[:, 0] + f[:, 1]) * np.float32(0.5))


def _mixed():
    rng = np.random.default_rng(99)
    recs = [signal(rng, 5000, 2, np.int16), signal(rng, 4410 + 7, 1, np.float32), signal(rng, 3 * TILE + 5, 3, np.float32),
            signal(rng, 2000, 1, np.int16), signal(rng, 1, 2, np.float32), signal(rng, 7000, 8, np.float32)]
    return recs, [48000, 44100, 16000, 8000, 11025, 96000]


def test_batch_invariance(fe):
    recs, rates = _mixed()
    got = fe.resample_16k(recs, rates)
    for r, (x, sr) in enumerate(zip(recs, rates)):
        alone = fe.resample_16k([x], [sr])[0]
        assert np.array_equal(alone.view(np.uint32), got[r].view(np.uint32)), "recording %d alone" % r
        # at another offset, behind other recordings of other rates
        shifted = fe.resample_16k([recs[(r + 1) % 6][:777], np.zeros(0, np.float32), x], [rates[(r + 1) % 6], 22050, sr])[2]
        assert np.array_equal(shifted.view(np.uint32), got[r].view(np.uint32)), "recording %d at another offset" % r
        if sr == 16000:
            assert np.array_equal(got[r], ref.downmix(x))
        else:
            m, want = reference(sr, x)
            assert np.abs(got[r] - want).max() <= gate(sr, m)


def test_batch_invariance_of_an_all_int16_batch(fe):
    """One dtype per call: the batch above reaches the kernel as f32.  Here every recording is int16, so the int16
    instantiation itself runs a multi-recording batch, recordings at non-zero offsets."""
    rng = np.random.default_rng(7)
    recs = [signal(rng, 5000, 2, np.int16), signal(rng, 4410 + 7, 1, np.int16), signal(rng, 2 * TILE + 5, 3, np.int16),
            signal(rng, 0, 1, np.int16), signal(rng, 2000, 1, np.int16), signal(rng, 3000, 8, np.int16)]
    rates = [48000, 44100, 16000, 32000, 8000, 96000]
    assert B._pack_interleaved(recs, rates)[0].dtype == np.int16
    got = fe.resample_16k(recs, rates)
    for r, (x, sr) in enumerate(zip(recs, rates)):
        alone = fe.resample_16k([x], [sr])[0]
        assert np.array_equal(alone.view(np.uint32), got[r].view(np.uint32)), "recording %d alone" % r
        shifted = fe.resample_16k([recs[(r + 1) % 6][:333], x], [rates[(r + 1) % 6], sr])[1]
        assert np.array_equal(shifted.view(np.uint32), got[r].view(np.uint32)), "recording %d at another offset" % r
        as_f32 = fe.resample_16k([x.astype(np.float32) / np.float32(32768)], [sr])[0]      # the f32 instantiation: same bits
        assert np.array_equal(as_f32.view(np.uint32), got[r].view(np.uint32)), "recording %d as f32" % r


def test_host_and_device_memory_give_the_same_bits(fe):
    recs, rates = _mixed()
    host = fe.resample_16k(recs, rates)
    ptr, offs = fe.resample_16k(recs, rates, device=True)
    try:
        dev = fe.download(ptr, (int(offs[-1]),), np.float32)
    finally:
        fe.dev_free(ptr)
    assert [int(o) for o in np.diff(offs)] == [h.size for h in host]
    for r, h in enumerate(host):
        assert np.array_equal(dev[offs[r]:offs[r + 1]].view(np.uint32), h.view(np.uint32)), r
    # a spanned sub-range of a larger host array: only those samples are read
    pcm, eo, ch, sr = B._pack_interleaved(recs, rates)
    pad = np.concatenate([np.full(1001, np.nan, np.float32), pcm, np.full(13, np.nan, np.float32)])
    eo2 = eo + 1001
    out = np.empty(int(offs[-1]), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert fe.lib.wm_resample_16k(fe.handle, p(pad), 1, p(eo2), p(ch), p(sr), len(recs), p(out), 0) == 0
    assert np.array_equal(out.view(np.uint32), dev.view(np.uint32))


def test_device_output_chains_into_logmel_long(fe):
    recs, rates = _mixed()
    ptr, offs = fe.resample_16k(recs, rates, device=True)
    try:
        pcm16 = fe.download(ptr, (int(offs[-1]),), np.float32)
        d_mel, mel_offs, T = fe.logmel_long_device(ptr, np.float32, offs)
        try:
            mel = fe.download(d_mel, (int(mel_offs[-1]),), np.float32)
        finally:
            fe.dev_free(d_mel)
    finally:
        fe.dev_free(ptr)
    assert [int(o) for o in offs] == [0] + list(np.cumsum([B.resample_out_len(len(x), sr) for x, sr in zip(recs, rates)]))
    want = fe.logmel_long([pcm16[offs[r]:offs[r + 1]] for r in range(len(recs))])
    for r, w in enumerate(want):
        assert np.array_equal(mel[mel_offs[r]:mel_offs[r + 1]].reshape(80, T[r]), w), r


def test_rejections(fe):
    lib, h = fe.lib, fe.handle
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pcm = np.zeros(4000, np.float32)
    out = np.zeros(8000, np.float32)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def call(pcm_p=p(pcm), dtype=1, offs=i64(0, 3000), ch=i32(2), sr=i32(48000), R=1, out_p=p(out), mem=0):
        return lib.wm_resample_16k(h, pcm_p, dtype, p(offs) if offs is not None else None, p(ch) if ch is not None else None,
                                   p(sr) if sr is not None else None, R, out_p, mem)

    assert call() == 0
    assert call(offs=i64(0, 3001)) == WM_ERR_INVALID and b"multiple" in lib.wm_last_error()
    assert call(ch=i32(0)) == WM_ERR_INVALID and call(ch=i32(9)) == WM_ERR_INVALID
    for bad in (44101, 3999, 200000):
        assert call(sr=i32(bad)) == WM_ERR_INVALID and str(bad).encode() in lib.wm_last_error()
    assert call(dtype=2) == WM_ERR_INVALID and call(dtype=3) == WM_ERR_INVALID           # WM_F64, WM_BF16
    assert call(pcm_p=None) == WM_ERR_INVALID and call(out_p=None) == WM_ERR_INVALID
    assert call(offs=None) == WM_ERR_INVALID and call(ch=None) == WM_ERR_INVALID and call(sr=None) == WM_ERR_INVALID
    assert call(offs=i64(3000, 0)) == WM_ERR_INVALID and call(offs=i64(-2, 0)) == WM_ERR_INVALID
    assert call(offs=i64(0, 2000, 1000), ch=i32(1, 1), sr=i32(48000, 48000), R=2) == WM_ERR_INVALID
    assert call(R=-1) == WM_ERR_INVALID and call(R=65536) == WM_ERR_INVALID
    assert call(R=0, pcm_p=None, offs=None, ch=None, sr=None, out_p=None) == 0             # nothing to do is legal
    assert call(pcm_p=None, offs=i64(0, 0), out_p=None) == 0                               # one empty recording


# ---------------------------------------------------------------- end to end
SOT, TASK, SOT_PREV, NS, TSB, EOT = 50258, 50359, 50361, 50362, 50364, 50257


@pytest.fixture(scope="module")
def prod(pkg):
    """The lively tiny model of tests/test_longform_gpu.py: production vocabulary, a short text context."""
    dims = dict(R.TINY_DIMS, n_vocab=51865, n_text_ctx=64)
    ctx = pkg.binding.Context(dims)
    ctx.init_synthetic(29)
    _perturb_ln_on_device(ctx, dims, seed=6)
    _lively_on_device(ctx, dims)
    ctx.finalize()
    ctx.set_suppress([SOT, SOT_PREV, NS, 50363, 50358], [220, EOT])
    yield ctx
    ctx.close()


def test_transcribe_long_from_48k_stereo_and_44k1_mono(prod):
    t48 = np.arange(4 * 48000, dtype=np.float64) / 48000
    t44 = np.arange(int(3.3 * 44100), dtype=np.float64) / 44100
    env = lambda t: 0.5 + 0.5 * np.sin(2 * np.pi * 0.37 * t)
    left = 0.3 * np.sin(2 * np.pi * 310 * t48) * env(t48)
    right = 0.2 * np.sin(2 * np.pi * 523 * t48) * env(t48)
    a = np.round(np.stack([left, right], axis=1) * 32767).astype(np.int16)
    b = (0.3 * np.sin(2 * np.pi * 440 * t44) * env(t44)).astype(np.float32)
    kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, lang_first=50259, lang_last=50357)
    got = prod.transcribe_long([a, b], sample_rates=[48000, 44100], **kw)
    pcm = prod.resample_16k([a, b], [48000, 44100])
    assert [x.size for x in pcm] == [4 * 16000, ref.out_len(len(b), 44100)]
    want = prod.transcribe_long(pcm, **kw)
    for g, w in zip(got, want):
        assert g["language"] == w["language"] and g["seeks"] == w["seeks"] and g["segments"] == w["segments"]
        assert [x["tokens"] for x in g["windows"]] == [x["tokens"] for x in w["windows"]]
        assert len(g["windows"]) >= 1
