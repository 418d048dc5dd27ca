"""GPU tests of the multichannel front: wm_resample_16k_mix (csrc/resample.hip) and wm_channel_activity
(csrc/channel_activity.hip) against the f64 restatement tests/channels_ref.py, and transcribe_long(channels=...) end to end.

Gates, derived, not measured.  The mix kernel: |y - y_ref| <= (T + 2 + C) * 2^-24 * 2.23 * A, A = max_k sum_c |w_c| |x_c[k]|, T
the rate's taps per output -- test_resample_gpu.py's bound plus one rounding per channel of the mix; at 16000 Hz the output
is the mixed sample itself: C * 2^-24 * A.  The activity: |a - a_ref| <= 160 * 2^-24 * a_ref against the f64 sum of the very
f32 samples given -- 159 additions of non-negative terms in any order.  Every comparison prints the worst ratio it saw."""
import ctypes
import importlib

import numpy as np
import pytest

import channels_ref as cref
import resample_ref as ref
from test_resample_gpu import EOT, NS, SOT, TASK, TILE, TSB, fe, frames_for_outputs, lengths, prod, signal  # noqa: F401 (fixtures)

B = importlib.import_module("openai_whisper_coreml_amd.binding")

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1
RATES = (48000, 44100, 8000, 16000)     # L = 1, L > 1, upsampling, the bypass
ACT_TILE = 64                           # frames per workgroup (csrc/wm_internal.h WM_CHANACT_TILE)
_H = {}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def prototype(sr):
    if sr not in _H and sr != 16000:
        _H[sr] = ref.prototype(sr)[0]
    return _H.get(sr)


def mix_gate(sr, C, A):
    if sr == 16000:
        return C * 2.0 ** -24 * A
    return (ref.taps(sr) + 2 + C) * 2.0 ** -24 * 2.23 * A


def weights(rng, n_rows, C):
    w = rng.uniform(-1.0, 1.0, size=(n_rows, C)).astype(np.float32)
    w.flat[0] = 1.0 if (n_rows + C) % 2 else -1.0       # the ends of the range too
    return w


def frames(x):
    return np.asarray(x).reshape(len(x), -1)


# ---------------------------------------------------------------- the mix kernel against f64
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("sr", RATES)
def test_mix_rates_lengths_channels_and_rows_against_the_f64_restatement(fe, sr, dtype):
    rng = np.random.default_rng(31 * sr + (1 if dtype == np.int16 else 0))
    lens = lengths(sr) if sr != 16000 else [0, 1, 2, TILE - 1, TILE, TILE + 1, 5000]
    shapes = [(1, 1), (2, 2), (3, 3), (8, 8), (2, 1), (1, 8), (8, 3), (3, 2)]          # (C, n_rows): both cover 1, 2, 3, 8
    recs, mats = [], []
    for i, n in enumerate(lens):
        for k in range(3):                                    # three shapes per length; every shape meets every length class
            C, n_rows = shapes[(3 * i + k) % len(shapes)]
            recs.append(signal(rng, n, C, dtype))
            mats.append(weights(rng, n_rows, C))
    got = fe.resample_16k_mix(recs, [sr] * len(recs), mats)
    worst = 0.0
    for x, w, sigs in zip(recs, mats, got):
        C = w.shape[1]
        assert len(sigs) == w.shape[0]
        for o, y in enumerate(sigs):
            want = cref.resample_mix(x, sr, w[o], prototype(sr))
            assert y.dtype == np.float32 and y.shape == want.shape == (ref.out_len(len(x), sr),)
            if not y.size:
                continue
            A = cref.mix_scale(x, w[o])
            err = float(np.abs(y - want).max())
            worst = max(worst, err / max(mix_gate(sr, C, A), 1e-300))
            assert err <= mix_gate(sr, C, A), "rate %d, %r %s, row %d of %r: max|err| %g > gate %g" % (
                sr, np.shape(x), np.dtype(dtype).name, o, w.shape, err, mix_gate(sr, C, A))
    print("mix rate %d %s: taps %d, worst max|err| / gate = %.3f" % (sr, np.dtype(dtype).name, ref.taps(sr) if sr != 16000 else 0, worst))


# ---------------------------------------------------------------- exact anchors to the code that exists
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_a_one_hot_row_is_resample_16k_on_that_channel_as_a_mono_recording(fe, dtype):
    rng = np.random.default_rng(5)
    for sr in RATES:
        for C in (2, 3, 8):
            x = signal(rng, frames_for_outputs(sr, TILE + 9) if sr != 16000 else TILE + 9, C, dtype)
            if dtype == np.float32:
                x[7, :] = -0.0
            got = fe.resample_16k_mix([x], [sr], [B.channel_rows("split", C)])[0]
            mono = fe.resample_16k([np.ascontiguousarray(x[:, c]) for c in range(C)], [sr] * C)
            for c in range(C):
                one = fe.resample_16k_mix([x], [sr], [B.channel_rows(c, C)])[0][0]
                assert np.array_equal(u32(one), u32(got[c])), (sr, C, c)
                if sr == 16000:      # as values: a -0.0 sample may come out +0.0
                    assert np.array_equal(got[c], mono[c]), (sr, C, c)
                else:
                    assert np.array_equal(u32(got[c]), u32(mono[c])), (sr, C, c)


def test_the_int16_stereo_row_of_halves_is_the_mean_bit_for_bit(fe):
    rng = np.random.default_rng(6)
    for sr in RATES:
        x = signal(rng, 5000, 2, np.int16)
        got = fe.resample_16k_mix([x], [sr], [np.array([[0.5, 0.5]], np.float32)])[0][0]
        mean = fe.resample_16k([x], [sr])[0]
        assert np.array_equal(u32(got), u32(mean)), sr
        assert np.array_equal(u32(fe.resample_16k_mix([x], [sr], [B.channel_rows("mean", 2)])[0][0]), u32(mean)), sr


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
def test_a_weighted_impulse_gives_the_weighted_slice_of_the_filter(fe, sr):
    h, L, M, K = B.resample_filter(sr)
    N = 3000
    n = np.arange(ref.out_len(N, sr), dtype=np.int64)
    for w, k, c in ((0.5, 0, 0), (-2.0, 1, 1), (0.25, N - 2, 2), (1.0, N - 1, 1)):
        x = np.zeros((N, 3), np.float32)
        x[k, c] = 1.0
        row = np.zeros((1, 3), np.float32)
        row[0, c] = w
        y = fe.resample_16k_mix([x], [sr], [row])[0][0]
        j = n * M - k * L
        want = np.float32(w) * np.where(np.abs(j) <= K, h[np.clip(j + K, 0, 2 * K)], np.float32(0))
        assert np.array_equal(y, want), "rate %d, impulse at %d"  % (sr, k)      # w a power of two: one exact product per output
        assert np.count_nonzero(y) > 0


# ---------------------------------------------------------------- invariance, bitwise
def _batch(dtype=None):
    rng = np.random.default_rng(77)
    dt = lambda d: dtype or d
    recs = [signal(rng, 5000, 2, dt(np.int16)), signal(rng, 4410 + 7, 3, dt(np.float32)), signal(rng, 2 * TILE + 5, 3, dt(np.float32)),
            signal(rng, 2000, 1, dt(np.int16)), signal(rng, 1, 2, dt(np.float32)), signal(rng, 3000, 8, dt(np.float32))]
    rates = [48000, 44100, 16000, 8000, 11025, 96000]
    mats = [weights(rng, n, frames(x).shape[1]) for n, x in zip((2, 3, 1, 2, 8, 3), recs)]
    return recs, rates, mats


@pytest.mark.parametrize("dtype", [None, np.int16])
def test_a_signal_is_the_same_bits_alone_batched_reordered_and_shifted(fe, dtype):
    recs, rates, mats = _batch(dtype)
    pcm_dtype = B._pack_interleaved(recs, rates)[0].dtype
    assert pcm_dtype == (np.int16 if dtype is not None else np.float32)      # both instantiations meet a multi-recording launch
    got = fe.resample_16k_mix(recs, rates, mats)
    for r, (x, sr, w) in enumerate(zip(recs, rates, mats)):
        alone = fe.resample_16k_mix([x], [sr], [w])[0]
        flipped = fe.resample_16k_mix([x], [sr], [w[::-1]])[0][::-1]                           # its rows in another order
        q = (r + 1) % len(recs)
        shifted = fe.resample_16k_mix([recs[q][:777], x[:0], x], [rates[q], 22050, sr], [mats[q], w[:1], w])[2]   # another offset
        for o in range(len(w)):
            single = fe.resample_16k_mix([x], [sr], [w[o:o + 1]])[0][0]                        # without the rows in front of it
            for name, other in (("alone", alone[o]), ("rows reversed", flipped[o]), ("shifted", shifted[o]), ("single row", single)):
                assert np.array_equal(u32(other), u32(got[r][o])), "recording %d row %d: %s" % (r, o, name)


def test_host_and_device_memory_give_the_same_bits(fe):
    recs, rates, mats = _batch()
    host = [y for sigs in fe.resample_16k_mix(recs, rates, mats) for y in sigs]
    ptr, offs = fe.resample_16k_mix(recs, rates, mats, device=True)
    try:
        dev = fe.download(ptr, (int(offs[-1]),), np.float32)
    finally:
        fe.dev_free(ptr)
    assert [int(o) for o in np.diff(offs)] == [y.size for y in host] and len(offs) == sum(len(m) for m in mats) + 1
    for s, y in enumerate(host):
        assert np.array_equal(u32(dev[offs[s]:offs[s + 1]]), u32(y)), s
    # a spanned sub-range of a larger host array: only those samples are read
    pcm, eo, ch, sr = B._pack_interleaved(recs, rates)
    rows, flat = B._pack_mix(mats, ch)
    pad = np.concatenate([np.full(1001, np.nan, np.float32), pcm, np.full(13, np.nan, np.float32)])
    eo2 = eo + 1001
    out = np.empty(int(offs[-1]), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert fe.lib.wm_resample_16k_mix(fe.handle, p(pad), 1, p(eo2), p(ch), p(sr), len(recs), p(rows), p(flat), p(out), 0) == 0
    assert np.array_equal(u32(out), u32(dev))


def test_device_output_of_a_two_row_call_chains_into_logmel_long(fe):
    rng = np.random.default_rng(8)
    recs = [signal(rng, 5000, 2, np.int16), signal(rng, 4410 + 7, 3, np.float32)]
    rates = [48000, 44100]
    mats = [B.channel_rows("split", 2), np.array([[1, 0, 0], [0.25, 0.5, -0.25]], np.float32)]
    ptr, offs = fe.resample_16k_mix(recs, rates, mats, device=True)
    try:
        pcm16 = fe.download(ptr, (int(offs[-1]),), np.float32)
        d_mel, mel_offs, T = fe.logmel_long_device(ptr, np.float32, offs)
        try:
            mel = fe.download(d_mel, (int(mel_offs[-1]),), np.float32)
        finally:
            fe.dev_free(d_mel)
    finally:
        fe.dev_free(ptr)
    lens = [B.resample_out_len(len(x), sr) for x, sr in zip(recs, rates)]
    assert [int(o) for o in offs] == [0] + list(np.cumsum([lens[0]] * 2 + [lens[1]] * 2))
    want = fe.logmel_long([pcm16[offs[s]:offs[s + 1]] for s in range(4)])
    for s, w in enumerate(want):
        assert np.array_equal(mel[mel_offs[s]:mel_offs[s + 1]].reshape(80, T[s]), w), s


# ---------------------------------------------------------------- the activity
def _act_lengths():
    return [0, 1, 159, 160, 161, 160 * 7 + 37, 160 * (ACT_TILE - 1), 160 * ACT_TILE, 160 * (ACT_TILE + 1), 160 * ACT_TILE + 1,
            160 * 2 * ACT_TILE + 159]


def test_activity_against_the_f64_sum_and_its_own_order(fe):
    rng = np.random.default_rng(9)
    sigs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in _act_lengths()] + [np.zeros(500, np.float32), np.zeros(0, np.float32)]
    got = fe.channel_activity(sigs)
    worst = 0.0
    for y, a in zip(sigs, got):
        want = cref.activity(y)
        assert a.dtype == np.float32 and a.shape == want.shape == (-(-len(y) // 160),)
        assert np.all(np.abs(a - want) <= 160 * 2.0 ** -24 * want), len(y)
        if a.size and want.max() > 0:
            worst = max(worst, float((np.abs(a - want) / np.maximum(want, 1e-30)).max()) / (160 * 2.0 ** -24))
        assert np.array_equal(u32(a), u32(cref.activity_f32(y))), len(y)       # the order the header states, bit for bit
    assert np.array_equal(got[-2], np.zeros(4, np.float32)) and got[-1].size == 0
    print("activity: worst |a - a_ref| / a_ref / gate = %.4f" % worst)


def test_a_nan_stays_in_its_frame(fe):
    y = np.full(160 * (ACT_TILE + 2) + 40, 0.25, np.float32)
    for k in (160 * 3 + 159, 160 * ACT_TILE, len(y) - 1):                     # a frame's last sample, a tile's first, the short frame
        z = y.copy()
        z[k] = np.nan
        a = fe.channel_activity([z])[0]
        f = k // 160
        assert np.isnan(a[f]) and np.all(np.isfinite(np.delete(a, f))), k
        assert np.array_equal(np.delete(a, f), np.delete(fe.channel_activity([y])[0], f))


def test_activity_is_the_same_bits_alone_batched_shifted_and_from_the_device(fe):
    rng = np.random.default_rng(10)
    sigs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in (160 * ACT_TILE + 77, 3, 0, 160 * 7 + 37, 4000)]
    got = fe.channel_activity(sigs)
    for s, y in enumerate(sigs):
        assert np.array_equal(u32(fe.channel_activity([y])[0]), u32(got[s])), s
        shifted = fe.channel_activity([sigs[(s + 1) % 5][:1237], y])[1]        # an offset that is no multiple of 4 or 160
        assert np.array_equal(u32(shifted), u32(got[s])), s
    offs = np.concatenate([[0], np.cumsum([len(y) for y in sigs])]).astype(np.int64)
    ptr = fe.to_device(np.concatenate(sigs))
    try:
        dev = fe.channel_activity(ptr, offs, device=True)
    finally:
        fe.dev_free(ptr)
    for s in range(5):
        assert np.array_equal(u32(dev[s]), u32(got[s])), s


# ---------------------------------------------------------------- rejections
def test_mix_rejections_leave_the_next_call_correct(fe):
    lib, h = fe.lib, fe.handle
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    rng = np.random.default_rng(11)
    x = signal(rng, 1500, 2, np.float32)
    w = weights(rng, 2, 2)
    good = fe.resample_16k_mix([x], [48000], [w])[0]
    pcm = np.ascontiguousarray(x.reshape(-1))
    out = np.zeros(2 * 500, np.float32)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    f32 = lambda *v: np.array(v, dtype=np.float32)

    def call(pcm_a=pcm, dtype=1, offs=i64(0, 3000), ch=i32(2), sr=i32(48000), R=1, rows=i32(2), mix=w.reshape(-1), out_a=out, mem=0):
        return lib.wm_resample_16k_mix(h, p(pcm_a), dtype, p(offs), p(ch), p(sr), R, p(rows), p(mix), p(out_a), mem)

    def still_good():
        assert call() == 0
        assert np.array_equal(u32(out[:500]), u32(good[0])) and np.array_equal(u32(out[500:]), u32(good[1]))
        out[:] = 0

    still_good()
    bad = [dict(offs=i64(0, 2999)), dict(ch=i32(0)), dict(ch=i32(9)), dict(sr=i32(44101)), dict(sr=i32(3999)), dict(dtype=2),
           dict(dtype=3), dict(pcm_a=None), dict(out_a=None), dict(offs=None), dict(ch=None), dict(sr=None), dict(offs=i64(3000, 0)),
           dict(offs=i64(-2, 0)), dict(R=-1), dict(R=65536),
           # its own: rows outside 1 .. 8, a null n_rows / mix, weights that are not finite
           dict(rows=i32(0)), dict(rows=i32(9), mix=np.zeros(18, np.float32)), dict(rows=i32(-1)), dict(rows=None), dict(mix=None),
           dict(mix=f32(1, np.nan, 0, 1)), dict(mix=f32(1, 0, np.inf, 1)), dict(mix=f32(1, 0, 0, -np.inf))]
    for kw in bad:
        assert call(**kw) == WM_ERR_INVALID, kw
        assert lib.wm_last_error()
        still_good()
    # more than 65535 signals: 8192 empty recordings of 8 rows each
    R = 8192
    assert call(offs=np.zeros(R + 1, np.int64), ch=np.ones(R, np.int32), sr=np.full(R, 48000, np.int32), R=R, rows=np.full(R, 8, np.int32),
                mix=np.ones(8 * R, np.float32)) == WM_ERR_INVALID
    still_good()
    assert call(offs=np.zeros(R + 1, np.int64), ch=np.ones(R, np.int32), sr=np.full(R, 48000, np.int32), R=R,
                rows=np.concatenate([np.full(R - 1, 8, np.int32), i32(7)]), mix=np.ones(8 * R, np.float32)) == 0       # 65535: legal
    assert call(R=0, pcm_a=None, offs=None, ch=None, sr=None, rows=None, mix=None, out_a=None) == 0            # nothing to do is legal
    assert call(pcm_a=None, offs=i64(0, 0), out_a=None) == 0                                                  # one empty recording
    still_good()
    for kw in (dict(mix=[np.ones((9, 2))]), dict(mix=[np.ones((2, 3))]), dict(mix=[np.full((1, 2), np.nan)]), dict(mix=[])):
        with pytest.raises(ValueError):
            fe.resample_16k_mix([x], [48000], **kw)


def test_activity_rejections_leave_the_next_call_correct(fe):
    lib, h = fe.lib, fe.handle
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    y = np.random.default_rng(12).uniform(-1, 1, 1000).astype(np.float32)
    good = fe.channel_activity([y[:700], y[700:]])
    out = np.zeros(7, np.float32)
    i64 = lambda *v: np.array(v, dtype=np.int64)

    def call(pcm=y, offs=i64(0, 700, 1000), S=2, out_a=out, mem=0):
        return lib.wm_channel_activity(h, p(pcm), p(offs), S, p(out_a), mem)

    def still_good():
        assert call() == 0
        assert np.array_equal(u32(out[:5]), u32(good[0])) and np.array_equal(u32(out[5:]), u32(good[1]))
        out[:] = 0

    still_good()
    for kw in (dict(offs=i64(0, 700, 699)), dict(offs=i64(-1, 700, 1000)), dict(offs=i64(800, 700, 1000)), dict(offs=None),
               dict(pcm=None), dict(out_a=None), dict(S=-1), dict(S=65536)):
        assert call(**kw) == WM_ERR_INVALID, kw
        assert lib.wm_last_error()
        still_good()
    assert call(S=0, pcm=None, offs=None, out_a=None) == 0
    assert call(pcm=None, offs=i64(5, 5, 5), out_a=None) == 0                  # empty signals are legal
    still_good()


# ---------------------------------------------------------------- end to end
def _recordings():
    """48 kHz int16 stereo, 4 s: a tone on the left in the first half, on the right in the second; and 44.1 kHz mono"""
    t48 = np.arange(4 * 48000, dtype=np.float64) / 48000
    t44 = np.arange(int(3.3 * 44100), dtype=np.float64) / 44100
    env = lambda t: 0.5 + 0.5 * np.sin(2 * np.pi * 0.37 * t)
    left = 0.3 * np.sin(2 * np.pi * 310 * t48) * (t48 < 2.0)
    right = 0.2 * np.sin(2 * np.pi * 523 * t48) * (t48 >= 2.0)
    a = np.round(np.stack([left, right], axis=1) * 32767).astype(np.int16)
    b = (0.3 * np.sin(2 * np.pi * 440 * t44) * env(t44)).astype(np.float32)
    return [a, b], [48000, 44100]


KW = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, lang_first=50259, lang_last=50357)


def _same_run(g, w):
    assert g["language"] == w["language"] and g["seeks"] == w["seeks"] and g["segments"] == w["segments"]
    assert [x["tokens"] for x in g["windows"]] == [x["tokens"] for x in w["windows"]]
    assert len(g["windows"]) >= 1


def test_transcribe_long_split_is_the_run_on_the_split_signals(prod):
    recs, rates = _recordings()
    got = prod.transcribe_long(recs, sample_rates=rates, channels="split", **KW)
    sigs = prod.resample_16k_mix(recs, rates, [B.channel_rows("split", 2), B.channel_rows("split", 1)])
    assert [[y.size for y in s] for s in sigs] == [[64000, 64000], [ref.out_len(len(recs[1]), 44100)]]
    want = prod.transcribe_long([y for s in sigs for y in s], **KW)
    assert [len(g["channels"]) for g in got] == [2, 1]
    for g, w in zip([ch for g in got for ch in g["channels"]], want):
        _same_run(g, w)
    for g in got:
        merged = sorted(([dict(sg, channel=c) for c, ch in enumerate(g["channels"]) for sg in ch["segments"]]),
                        key=lambda sg: (sg["start"], sg["channel"]))
        assert g["segments"] == merged


def test_transcribe_long_diarize_is_the_plain_run_with_speakers(prod):
    recs, rates = _recordings()
    got = prod.transcribe_long(recs, sample_rates=rates, channels="diarize", **KW)
    want = prod.transcribe_long(recs, sample_rates=rates, **KW)
    sigs = prod.resample_16k_mix(recs, rates, [B.channel_rows("split", 2), B.channel_rows("split", 1)])
    act = [prod.channel_activity(s) for s in sigs]
    assert [a.size for a in act[0]] == [400, 400]
    assert all(sg["speaker"] is None for sg in got[1]["segments"])                         # mono
    for g, w, a in zip(got, want, act):
        for sg in g["segments"]:
            assert sg.pop("speaker") == B.speaker_by_channel(a, sg["start"], sg["end"], 1.1)
        _same_run(g, w)
    # the rule on the recording itself, whatever the synthetic model emits
    assert B.speaker_by_channel(act[0], 0.2, 1.8) == 0 and B.speaker_by_channel(act[0], 2.2, 3.8) == 1
