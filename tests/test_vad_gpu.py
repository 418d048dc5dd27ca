"""GPU tests of the speech-activity path: wm_vad_energy (csrc/vad.hip) against the f64 restatement of tests/vad_ref.py on
wm_logmel_long's own output, its bit-level batch invariance, extents and argument checks, the segments of the reference
burst recording from the device energy, and transcribe_long(vad=..., parallel_clips=...) end to end on the lively tiny model
(tests/test_longform_gpu.py: prod) -- every end-to-end comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import vad_ref as V
from conftest import GOLDEN
from test_longform_cpu import long_log_mel_np
from test_longform_gpu import _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_vad_cpu import energy_tolerance, threshold_distance

pytestmark = pytest.mark.gpu

WM_OK, WM_ERR_INVALID = 0, 1
F = 224   # frames per workgroup of the kernel (include/whisper_mi355x.h)
# recordings of 0.3 - 3 s and the frames asked of each: nothing, one, a tile less one, a tile, a tile and one, two tiles and one
# (n_frames may reach into the padding: it is bounded by mel_len = content + 3000)
SECONDS = (0.3, 0.5, 2.23, 2.24, 2.6, 3.0)
N_FRAMES = (0, 1, F - 1, F, F + 1, 2 * F + 1)
TRIPLES = ((1, 2, 3), (3, 4, 5), (5, 0, 2))   # three recordings in one call, the first never at element 0


@pytest.fixture(scope="module")
def fe(pkg):
    ctx = pkg.binding.Context()
    yield ctx
    ctx.close()


def _recordings():
    rng = np.random.default_rng(8)
    out = []
    for k, s in enumerate(SECONDS):
        n = int(round(16000 * s))
        t = np.arange(n) / 16000.0
        x = 0.02 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * (300 + 170 * k) * t) * (t % 0.5 < 0.3)
        out.append(x.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def mels(fe):
    """n_mels -> (the flat log-mel of the six recordings on the host, the same on the device, offsets, T)."""
    out = {}
    for n_mels in (80, 128):
        ptr, offs, T = fe.logmel_long(_recordings(), n_mels=n_mels, device=True)
        out[n_mels] = (fe.download(ptr, (int(offs[-1]),), np.float32), ptr, offs, T)
    yield out
    for v in out.values():
        fe.dev_free(v[1])


def _call(fe, mels, n_mels, rows, band, smooth, device, raw=True, n_frames=None):
    host, ptr, offs, T = mels[n_mels]
    rows = list(rows)
    n = [N_FRAMES[r] for r in rows] if n_frames is None else n_frames
    return fe.vad_energy(ptr if device else host, offs[rows], T[rows], n, band, smooth, device=device, raw=raw, n_mels=n_mels)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n_mels", [80, 128])
def test_energy_against_the_f64_restatement(fe, mels, n_mels, device):
    """Gate: 2^-23 (n_band + smooth + 16) max(1, max|e_ref|).  Measured on an MI355X: see NOTEBOOK.md (the worst error over
    all cases as a fraction of its gate is printed)."""
    host, _, offs, T = mels[n_mels]
    worst = (0.0, 0.0, None)
    for band in ((0, n_mels), (17, 18), (n_mels // 4, n_mels // 4 + 37)):
        for smooth in (1, 5, 31):
            for rows in TRIPLES:
                raw, y = _call(fe, mels, n_mels, rows, band, smooth, device)
                y_only = _call(fe, mels, n_mels, rows, band, smooth, device, raw=False)   # raw_out null
                for k, r in enumerate(rows):
                    n = N_FRAMES[r]
                    assert raw[k].shape == y[k].shape == (n,)
                    assert np.array_equal(y_only[k], y[k])
                    if n == 0:
                        continue
                    mel = host[offs[r]:offs[r + 1]].reshape(n_mels, T[r])
                    e_ref, y_ref = V.energy_ref(mel, n, band[0], band[1], smooth)
                    tol = energy_tolerance(band[1] - band[0], smooth, e_ref)
                    err = max(float(np.abs(raw[k] - e_ref).max()), float(np.abs(y[k] - y_ref).max()))
                    if err / tol > worst[0]:
                        worst = (err / tol, err, (band, smooth, r))
                    assert err <= tol, (band, smooth, r, err, tol)
                    if smooth == 1:
                        assert np.array_equal(raw[k], y[k])
    print("wm_vad_energy %d mels %s: worst error %.3g = %.3f of its gate at %s" % (
        n_mels, "device" if device else "host", worst[1], worst[0], worst[2]))


def test_a_recording_is_bit_identical_alone_in_a_batch_and_at_another_offset(fe, mels):
    host, ptr, offs, T = mels[80]
    for band, smooth in (((0, 80), 5), ((2, 62), 31)):
        batch = _call(fe, mels, 80, range(6), band, smooth, True, n_frames=[2 * F + 1] * 6)
        from_host = _call(fe, mels, 80, range(6), band, smooth, False, n_frames=[2 * F + 1] * 6)
        shifted = np.concatenate([np.zeros(3, np.float32), host])   # every row at another alignment
        d = fe.to_device(shifted)
        try:
            moved = fe.vad_energy(d, offs[:6] + 3, T, [2 * F + 1] * 6, band, smooth, device=True, raw=True, n_mels=80)
        finally:
            fe.dev_free(d)
        for r in range(6):
            alone = _call(fe, mels, 80, [r], band, smooth, True, n_frames=[2 * F + 1])
            for k in (0, 1):
                assert np.array_equal(alone[k][0], batch[k][r]) and np.array_equal(from_host[k][r], batch[k][r])
                assert np.array_equal(moved[k][r], batch[k][r])
            # fewer frames of the same recording: the same values up to where the shorter window of the smoothing ends
            short = _call(fe, mels, 80, [r], band, smooth, True, n_frames=[F + 1])
            assert np.array_equal(short[0][0], batch[0][r][:F + 1])
            assert np.array_equal(short[1][0][:F + 1 - smooth // 2], batch[1][r][:F + 1 - smooth // 2])


def test_outputs_are_written_exactly_to_their_extents(fe, mels, pkg):
    b = pkg.binding
    host, ptr, offs, T = mels[80]
    rows = [3, 0, 5]
    n = np.array([N_FRAMES[r] for r in rows], dtype=np.int32)
    total, CAN = int(n.sum()), 1024
    buf = np.full(2 * (total + 2 * CAN), 12345.0, dtype=np.float32)
    d = fe.to_device(buf)
    try:
        d_y = ctypes.c_void_p(d.value + 4 * CAN)
        d_e = ctypes.c_void_p(d.value + 4 * (total + 3 * CAN))
        base, Tr = np.ascontiguousarray(offs[rows]), np.ascontiguousarray(T[rows])
        assert fe.lib.wm_vad_energy(fe.handle, ptr, b._ptr(base), b._ptr(Tr), b._ptr(n), 3, 80, 0, 80, 31, d_e, d_y,
                                    b.WM_MEM_DEVICE) == WM_OK
        fe.sync()
        got = fe.download(d, buf.shape, np.float32).reshape(2, total + 2 * CAN)
    finally:
        fe.dev_free(d)
    for half in got:
        assert np.all(half[:CAN] == 12345.0) and np.all(half[CAN + total:] == 12345.0)
        assert not np.any(half[CAN:CAN + total] == 12345.0)


def test_invalid_arguments_are_rejected(fe, mels, pkg):
    b = pkg.binding
    host, ptr, offs, T = mels[80]
    y = np.zeros(4096, np.float32)

    def call(mel=host, base=(offs[1],), T_=(T[1],), n=(100,), R=1, n_mels=80, lo=0, hi=80, smooth=5, out=y, mem=b.WM_MEM_HOST):
        base, T_, n = np.array(base, np.int64), np.array(T_, np.int32), np.array(n, np.int32)
        return fe.lib.wm_vad_energy(fe.handle, None if mel is None else b._ptr(mel), b._ptr(base) if base.size else None,
                                    b._ptr(T_) if T_.size else None, b._ptr(n) if n.size else None, R, n_mels, lo, hi, smooth,
                                    None, None if out is None else b._ptr(out), mem)
    assert call() == WM_OK
    assert call(R=0, mel=None, base=(), T_=(), n=(), out=None) == WM_OK
    for bad in (dict(n_mels=64), dict(lo=-1), dict(lo=80, hi=80), dict(lo=40, hi=40), dict(lo=50, hi=40), dict(hi=81),
                dict(smooth=0), dict(smooth=4), dict(smooth=33), dict(smooth=-1), dict(n=(-1,)), dict(n=(int(T[1]) + 1,)),
                dict(T_=(0,), n=(0,)), dict(base=(-1,)), dict(mel=None), dict(out=None), dict(base=()), dict(T_=()), dict(n=()),
                dict(R=-1), dict(R=65536)):
        assert call(**bad) == WM_ERR_INVALID, bad


def test_non_finite_values_propagate(fe, mels):
    host, _, offs, T = mels[80]
    mel = host[offs[4]:offs[5]].copy()
    t_nan, t_inf = 50, 150
    mel[30 * T[4] + t_nan] = np.nan
    mel[31 * T[4] + t_inf] = np.inf
    e, y = fe.vad_energy(mel, [0], [T[4]], [F + 1], (0, 80), 5, raw=True, n_mels=80)
    bad_e = ~np.isfinite(e[0])
    assert list(np.flatnonzero(bad_e)) == [t_nan, t_inf] and np.isnan(e[0][t_nan])
    bad_y = ~np.isfinite(y[0])
    assert list(np.flatnonzero(bad_y)) == list(range(t_nan - 2, t_nan + 3)) + list(range(t_inf - 2, t_inf + 3))
    # outside the band they are not read
    e2, _ = fe.vad_energy(mel, [0], [T[4]], [F + 1], (32, 80), 5, raw=True, n_mels=80)
    assert np.isfinite(e2[0]).all()


def test_the_burst_recording_gives_the_reference_segments(fe, pkg):
    b = pkg.binding
    x = V.bursts()
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    ref = long_log_mel_np(x, m80)
    n = ref.shape[1] - 3000
    ptr, offs, T = fe.logmel_long([x], device=True)
    try:
        for smooth in (5, 11):
            e_ref, y_ref = V.energy_ref(ref, n, 0, 80, smooth)
            # the precondition of comparing decisions: no frame of the reference near a threshold
            assert threshold_distance(y_ref.astype(np.float32)) >= 100 * energy_tolerance(80, smooth, e_ref)
            y = fe.vad_energy(ptr, offs[:1], T, [n], (0, 80), smooth, device=True)[0]
            assert b.vad_segments(y) == V.BURST_SEGMENTS
    finally:
        fe.dev_free(ptr)


# ---------------------------------------------------------------- end to end
IDS = [7, 300]
ONCE = dict(temperatures=(0.0,))


def _speech_recs():
    """Two recordings of tone bursts over faint noise: three and two spans of activity."""
    tone = _long_recs()[2]
    rng = np.random.default_rng(9)
    out = []
    for seconds, spans in ((72.0, ((2.0, 9.0), (15.0, 20.5), (30.0, 66.0))), (38.0, ((1.0, 4.0), (20.0, 35.5)))):
        x = (0.0005 * rng.standard_normal(int(16000 * seconds))).astype(np.float32)
        for a, z in spans:
            x[int(16000 * a):int(16000 * z)] += tone[int(16000 * a):int(16000 * z)]
        out.append(x)
    return out


def _no_round(out):
    return [dict(o, windows=[{k: v for k, v in w.items() if k != "round"} for w in o["windows"]]) for o in out]


def _seeks_grow_within_every_clip(out):
    for o in out:
        last = {}
        for w in o["windows"]:
            assert w["clip"] not in last or w["seek"] > last[w["clip"]], o["seeks"]
            assert not last or w["clip"] >= max(last), o["windows"]
            last[w["clip"]] = w["seek"]


def test_vad_equals_the_run_with_its_clips_given(prod):  # noqa: F811
    recs = _speech_recs()
    got = prod.transcribe_long(recs, recording_ids=IDS, vad=True, **_kw())
    assert [len(o["vad_segments"]) for o in got] == [3, 2] and [len(o["vad_clips"]) for o in got] == [2, 2]
    times = [[v / 100.0 for ab in o["vad_clips"] for v in ab] for o in got]
    want = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=times, **_kw())
    for g, w in zip(got, want):
        assert {k: v for k, v in g.items() if not k.startswith("vad_")} == w
    assert sum(len(o["windows"]) for o in got) >= 4
    _seeks_grow_within_every_clip(got)
    # the silence between the clips is never decoded
    for o in got:
        assert all(any(a <= w["seek"] and w["seek"] + w["segment_size"] <= z for a, z in o["vad_clips"]) for w in o["windows"])


@pytest.mark.parametrize("reuse", [False, True])
def test_parallel_clips_equal_the_sequential_clip_run(prod, reuse):  # noqa: F811
    recs = _speech_recs()
    kw = _kw(vad=dict(max_frames=1000), reuse_encoder=reuse, **ONCE)   # every span its own clip: five lanes
    seq = prod.transcribe_long(recs, recording_ids=IDS, **kw)
    assert [len(o["vad_clips"]) for o in seq] == [3, 2]
    for n_lanes in (2, True):
        par = prod.transcribe_long(recs, recording_ids=IDS, parallel_clips=n_lanes, **kw)
        assert _no_round(par) == seq
        _seeks_grow_within_every_clip(par)
        rounds = max(w["round"] for o in par for w in o["windows"]) + 1
        assert rounds >= max(sum(w["clip"] == c for w in o["windows"]) for o in par for c in range(3))
    assert rounds < max(len(o["windows"]) for o in seq)   # five lanes at once: fewer rounds than the longest recording has windows
    assert any(len(o["windows"]) > len(o["vad_clips"]) for o in seq)   # a clip longer than one window is walked


def test_a_lane_equals_its_clip_alone_under_the_fallback_temperatures(prod):  # noqa: F811
    recs = _speech_recs()
    clips = [[0.0, 0.0, 2.0, 9.0, 15.0, 15.0, 30.0, 66.0], [1.0, 4.0, 20.0, 35.5]]   # recording 0: clips 0 and 2 are empty
    kw = _kw(logprob_threshold=0.0, language=50259)   # every window falls back: sampled rows
    par = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=clips, parallel_clips=True, **kw)
    assert any(t > 0 for o in par for w in o["windows"] for t in w["temperatures"])
    assert [sorted({w["clip"] for w in o["windows"]}) for o in par] == [[1, 3], [0, 1]]
    _seeks_grow_within_every_clip(par)
    for r, o in enumerate(par):
        for k in sorted({w["clip"] for w in o["windows"]}):
            alone = prod.transcribe_long([recs[r]], recording_ids=[IDS[r]], parallel_clips=True,
                                         clip_timestamps=[[0.0, 0.0] * k + clips[r][2 * k:2 * k + 2]], **kw)[0]
            mine = [w for w in _no_round([o])[0]["windows"] if w["clip"] == k]
            assert _no_round([alone])[0]["windows"] == mine, (r, k)
            seeks = {w["seek"] for w in mine}
            assert [dict(s, id=None) for s in alone["segments"]] == [dict(s, id=None) for s in o["segments"] if s["seek"] in seeks]
