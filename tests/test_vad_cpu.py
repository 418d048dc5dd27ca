"""CPU tests of the speech-activity path's host side: wm_vad_segments against the f64 restatement of tests/vad_ref.py and on
hand-made cases of every rule, vad_clips, vad_band, and transcribe_long's vad= / parallel_clips= on a scripted fake context
whose windows depend on (recording, seek) alone -- so that a clip decodes the same whichever round it is in."""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest

import vad_ref as V
from conftest import GOLDEN
from test_longform_clips_cpu import ClipCtx, _kw, _plain, _rec
from test_longform_cpu import long_log_mel_np
from test_longform_words_cpu import EOT, TB, vocab  # noqa: F401  (vocab: fixture)

B = importlib.import_module("openai_whisper_coreml_amd.binding")
WM_OK, WM_ERR_INVALID = 0, 1


def _params(**over):
    p = B.wm_vad_params()
    B.load_library().wm_vad_default_params(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _segments_raw(y, p, cap=None, stats=True):
    """One wm_vad_segments call: (status, count, pairs written, stats)."""
    lib = B.load_library()
    y = np.ascontiguousarray(y, dtype=np.float32)
    n = ctypes.c_int(-7)
    cap = 64 if cap is None else cap
    seg = np.full((max(cap, 1), 2), -1, dtype=np.int32)
    st = np.full(4, 7.0, dtype=np.float32)
    status = lib.wm_vad_segments(B._ptr(y) if y.size else None, y.size, ctypes.byref(p), B._ptr(seg) if cap else None, cap,
                                 ctypes.byref(n), B._ptr(st) if stats else None)
    return status, n.value, [(int(a), int(b)) for a, b in seg[:min(cap, max(n.value, 0))]], st


def _same_stats(a, b):
    return all((math.isnan(x) and math.isnan(y)) or float(x) == float(y) for x, y in zip(a, b))


# ---------------------------------------------------------------- wm_vad_segments against the restatement
def _track(rng, kind):
    if kind == "walk":
        return np.cumsum(rng.standard_normal(int(rng.integers(4, 400)))) * rng.choice([0.05, 0.3, 1.0])
    if kind == "tiny":
        return rng.standard_normal(int(rng.integers(0, 4)))
    if kind == "equal":
        return np.full(int(rng.integers(1, 200)), rng.standard_normal())
    # runs of silence and speech with noise on top; `ends`: in speech / in a pending silence shorter than min_silence
    parts, level = [], 0
    for _ in range(int(rng.integers(2, 9))):
        parts.append(np.full(int(rng.integers(1, 90)), 4.0 * level))
        level ^= 1
    if kind == "ends_in_speech":
        parts.append(np.full(int(rng.integers(1, 60)), 4.0))
    if kind == "ends_pending":
        parts += [np.full(int(rng.integers(30, 60)), 4.0), np.zeros(int(rng.integers(1, 6)))]
    y = np.concatenate(parts)
    return y + rng.choice([0.0, 0.2, 1.0]) * rng.standard_normal(y.size)


def _random_params(rng):
    qf = float(rng.choice([0.0, 0.1, 0.25, 0.4]))
    on = float(rng.choice([0.05, 0.3, 0.5, 0.8, 1.0]))
    return dict(q_floor=qf, q_peak=float(rng.choice([qf + 0.05, 0.7, 0.95, 1.0])), min_range=float(rng.choice([0.0, 0.3, 1.0, 5.0])),
                on_frac=on, off_frac=float(on * rng.choice([0.0, 0.5, 0.7, 1.0])), min_speech=int(rng.integers(0, 31)),
                min_silence=int(rng.integers(1, 41)), speech_pad=int(rng.integers(0, 31)))


def test_segments_equal_the_restatement_on_random_tracks():
    rng = np.random.default_rng(11)
    kinds = ("walk", "tiny", "equal", "runs", "ends_in_speech", "ends_pending")
    seen = dict(flat=0, spans=0, none=0, merged=0)
    for case in range(360):
        kind = kinds[case % len(kinds)]
        y = _track(rng, kind).astype(np.float32)
        over = {} if case % 5 == 0 else _random_params(rng)
        want, want_stats = V.segments_ref(y, over)
        status, n, got, stats = _segments_raw(y, _params(**over), cap=256)
        assert status == WM_OK, (case, kind, B.load_library().wm_last_error())
        assert n == len(want) and got == want, (case, kind, over, got, want)
        assert _same_stats(stats, want_stats), (case, kind, over, stats, want_stats)
        assert B.vad_segments(y, over) == want
        if y.size and math.isnan(float(want_stats[2])):
            seen["flat"] += 1
        elif want:
            seen["spans"] += 1
            seen["merged"] += len(want) > 1
        else:
            seen["none"] += 1
    assert min(seen.values()) >= 10, seen   # every outcome is among the cases


# ---------------------------------------------------------------- one hand-made case per rule
def _steps(*runs):
    """(length, level) runs -> a track; level 0 = silence, 10 = speech."""
    return np.concatenate([np.full(n, float(v), dtype=np.float32) for n, v in runs])


HAND = dict(q_floor=0.0, q_peak=1.0, min_range=0.6, on_frac=0.5, off_frac=0.35, min_speech=25, min_silence=50, speech_pad=0)


def _hand(y, **over):
    p = dict(HAND)
    p.update(over)
    got, stats = B.vad_segments(y, p, stats=True)
    assert got == V.segments_ref(y, p)[0]
    return got, stats


def test_flat_track_is_one_segment_with_nan_thresholds():
    y = _steps((300, 1.0)) + np.float32(0.1) * np.sin(np.arange(300, dtype=np.float32))
    got, stats = _hand(y)
    assert got == [(0, 300)]
    assert stats[1] - stats[0] < 0.6 and math.isnan(stats[2]) and math.isnan(stats[3])
    # the same shape with contrast is cut
    assert _hand(_steps((100, 0), (100, 10), (100, 0)))[0] == [(100, 200)]


def test_thresholds_are_fractions_of_the_quantile_range():
    got, stats = _hand(_steps((100, 2), (100, 10), (100, 2)))
    assert stats == (2.0, 10.0, 6.0, float(np.float32(2.0 + float(np.float32(0.35)) * 8.0)))


def test_a_blip_shorter_than_min_speech_is_dropped():
    assert _hand(_steps((100, 0), (24, 10), (100, 0), (25, 10), (100, 0)))[0] == [(224, 249)]
    # ... also one that is still open at the end
    assert _hand(_steps((100, 0), (60, 10), (100, 0), (24, 10)))[0] == [(100, 160)]
    assert _hand(_steps((100, 0), (60, 10), (100, 0), (25, 10)))[0] == [(100, 160), (260, 285)]


def test_a_gap_shorter_than_min_silence_does_not_split():
    assert _hand(_steps((100, 0), (60, 10), (49, 0), (60, 10), (100, 0)))[0] == [(100, 269)]
    assert _hand(_steps((100, 0), (60, 10), (50, 0), (60, 10), (100, 0)))[0] == [(100, 160), (210, 270)]
    # a pending end that the recording's end cuts short keeps the span open to the end
    assert _hand(_steps((100, 0), (60, 10), (49, 0)))[0] == [(100, 209)]
    # between the thresholds: neither opens a span nor ends one, and does not cancel a pending end
    mid = 4.5   # thr_off 3.5 <= 4.5 < thr_on 5
    assert _hand(_steps((100, 0), (60, mid), (100, 0), (60, 10), (100, 0)))[0] == [(260, 320)]
    assert _hand(_steps((100, 0), (60, 10), (30, 0), (30, mid), (100, 0)))[0] == [(100, 160)]


def test_pad_is_clipped_at_both_ends():
    y = _steps((10, 0), (60, 10), (100, 0), (60, 10), (5, 0))
    assert _hand(y)[0] == [(10, 70), (170, 235)]   # (the last span is open at the end: the pending end never matures)
    assert _hand(y, speech_pad=40)[0] == [(0, 90), (150, 235)]
    assert _hand(y, speech_pad=41)[0] == [(0, 90), (150, 235)]   # speech_pad / 2 per side, integer division


def test_padded_spans_that_touch_are_merged():
    y = _steps((100, 0), (60, 10), (60, 0), (60, 10), (100, 0))
    assert _hand(y)[0] == [(100, 160), (220, 280)]
    assert _hand(y, speech_pad=58)[0] == [(71, 189), (191, 309)]
    assert _hand(y, speech_pad=60)[0] == [(70, 310)]   # start == the predecessor's end: merged


def test_cap_zero_sizes_and_a_small_cap_truncates():
    y = _steps((100, 0), (60, 10), (60, 0), (60, 10), (100, 0))
    p = _params(**HAND)
    assert _segments_raw(y, p, cap=0, stats=False)[:3] == (WM_OK, 2, [])
    assert _segments_raw(y, p, cap=1)[:3] == (WM_OK, 2, [(100, 160)])
    assert _segments_raw(np.zeros(0, np.float32), p, cap=4)[:3] == (WM_OK, 0, [])


def test_defaults():
    assert B.vad_default_params() == {k: (float(np.float32(v)) if k in V.FLOAT_FIELDS else v) for k, v in V.DEFAULTS.items()}
    B.load_library().wm_vad_default_params(None)   # a null pointer is a no-op


@pytest.mark.parametrize("over", [
    dict(q_floor=-0.1), dict(q_floor=0.95), dict(q_floor=0.96), dict(q_peak=1.1), dict(q_floor=math.nan), dict(q_peak=math.nan),
    dict(on_frac=0.0, off_frac=0.0), dict(on_frac=1.1), dict(off_frac=-0.1), dict(off_frac=0.6), dict(on_frac=math.nan),
    dict(off_frac=math.nan), dict(min_range=-1.0), dict(min_range=math.inf), dict(min_range=math.nan), dict(min_silence=0),
    dict(min_speech=-1), dict(speech_pad=-1)])
def test_invalid_parameters(over):
    y = _steps((100, 0), (60, 10), (100, 0))
    assert _segments_raw(y, _params(**over))[0] == WM_ERR_INVALID


def test_invalid_tracks_and_pointers():
    lib = B.load_library()
    y = _steps((100, 0), (60, 10), (100, 0))
    p = _params()
    bad = y.copy()
    bad[17] = np.nan
    assert _segments_raw(bad, p)[0] == WM_ERR_INVALID
    with pytest.raises(B.WhisperError):
        B.vad_segments(bad)
    n = ctypes.c_int(0)
    seg = np.zeros((4, 2), np.int32)
    assert lib.wm_vad_segments(None, 10, ctypes.byref(p), B._ptr(seg), 4, ctypes.byref(n), None) == WM_ERR_INVALID
    assert lib.wm_vad_segments(B._ptr(y), y.size, None, B._ptr(seg), 4, ctypes.byref(n), None) == WM_ERR_INVALID
    assert lib.wm_vad_segments(B._ptr(y), y.size, ctypes.byref(p), None, 4, ctypes.byref(n), None) == WM_ERR_INVALID
    assert lib.wm_vad_segments(B._ptr(y), y.size, ctypes.byref(p), B._ptr(seg), 4, None, None) == WM_ERR_INVALID
    assert lib.wm_vad_segments(B._ptr(y), -1, ctypes.byref(p), B._ptr(seg), 4, ctypes.byref(n), None) == WM_ERR_INVALID
    assert lib.wm_vad_segments(B._ptr(y), y.size, ctypes.byref(p), B._ptr(seg), -1, ctypes.byref(n), None) == WM_ERR_INVALID
    with pytest.raises(ValueError):
        B.vad_segments(y, dict(no_such_field=1))
    # +-inf are values like any other
    inf = y.copy()
    inf[:5], inf[130] = -np.inf, np.inf
    assert _segments_raw(inf, _params(q_floor=0.1, q_peak=0.8))[0] == WM_OK


# ---------------------------------------------------------------- vad_clips, vad_band
def test_clips_merge_up_to_max_frames():
    segs = [(0, 100), (200, 2900), (2950, 3000), (3001, 3100), (9000, 13000), (13010, 13020), (13030, 16010)]
    want = [(0, 3000), (3001, 3100), (9000, 13000), (13010, 16010)]
    assert B.vad_clips(segs) == want == V.clips_ref(segs)
    assert B.vad_clips(segs, max_frames=100) == V.clips_ref(segs, 100) == [
        (0, 100), (200, 2900), (2950, 3000), (3001, 3100), (9000, 13000), (13010, 13020), (13030, 16010)]
    assert B.vad_clips([]) == []
    assert B.vad_clips([(5, 4000)]) == [(5, 4000)]   # an over-long span stays one clip
    rng = np.random.default_rng(3)
    for _ in range(50):
        cuts = np.sort(rng.choice(20000, size=2 * int(rng.integers(0, 12)), replace=False))
        segs = [(int(a), int(b)) for a, b in cuts.reshape(-1, 2)]
        mf = int(rng.choice([1, 500, 3000]))
        assert B.vad_clips(segs, mf) == V.clips_ref(segs, mf)


@pytest.mark.parametrize("n_mels, want", [(80, (2, 62)), (128, (4, 100))])
def test_band_of_the_slaney_centres(n_mels, want):
    c = V.slaney_centres(n_mels)
    lo, hi = B.vad_band(n_mels)
    assert (lo, hi) == want
    assert all((100.0 <= f <= 4000.0) == (lo <= m < hi) for m, f in enumerate(c))
    assert B.vad_band(n_mels, 0.0, 8000.0) == (0, n_mels)
    inside = [m for m, f in enumerate(c) if 300.0 <= f <= 3400.0]
    assert B.vad_band(n_mels, 300.0, 3400.0) == (inside[0], inside[-1] + 1)
    with pytest.raises(ValueError):
        B.vad_band(n_mels, 101.0, 102.0)


def test_band_centres_are_the_filterbanks_peaks():
    """The 80-mel filterbank of the front end peaks at the bin nearest to each centre (its DFT bins are 40 Hz apart)."""
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    c = V.slaney_centres(80)
    assert all(abs(int(np.argmax(m80[m])) * 40.0 - c[m]) <= 40.0 for m in range(80))


# ---------------------------------------------------------------- transcribe_long on a fake context
WINDOWS = (
    [TB, 0, 1, TB + 200, TB + 200, 2],               # open end: the seek follows the last timestamp pair, 400 frames
    [TB, 0, 1, TB + 500],                            # closed by one timestamp: the seek takes the whole window
    [TB + 10, 0, TB + 300, TB + 300, 1, TB + 450, TB + 450],   # ends in a pair: 900 frames
    None,                                            # skipped by the no-speech rule
    [TB, 2, TB + 150, TB + 150, 1],                  # 300 frames
    [0, 1, 2],                                       # no timestamp at all
    [TB + 5, 1, 1, TB + 350, TB + 350, 0, 2],        # 700 frames
)


class VadCtx(ClipCtx):
    """ClipCtx whose window is a function of (recording, seek) -- not of the sample id -- plus scripted energy tracks."""

    def __init__(self, tracks=None, hot=()):
        ClipCtx.__init__(self, {})
        self.tracks = tracks
        self.hot = set(hot)   # (recording, seek) accepted only at temperature 0.6
        self.bases = None

    def logmel_long(self, recordings, n_mels=80, device=False):
        r = ClipCtx.logmel_long(self, recordings, n_mels, device)
        self.bases = [int(b) for b in r[1][:-1]]
        return r

    def vad_energy(self, mel, mel_offs, T, n_frames, band, smooth=5, device=False, raw=False, n_mels=None):
        self.calls.append(("vad_energy", _plain(mel_offs), _plain(T), _plain(n_frames), _plain(band), smooth, device, raw))
        assert [len(t) for t in self.tracks] == [int(n) for n in n_frames]
        return [np.asarray(t, dtype=np.float32) for t in self.tracks]

    def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **kw):
        self.calls.append(("transcribe_mel", _plain(mel_base), _plain(mel_len), _plain(seek), _plain(n_frames),
                           [_plain(p) for p in prompts], max_new, sorted((k, _plain(v)) for k, v in kw.items())))
        eot, t = kw["eot"], kw["temperature"]
        n = len(seek)
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.full(n, 0.01, dtype=np.float32)
        for i in range(n):
            rec = self.bases.index(int(mel_base[i]))
            w = WINDOWS[(int(seek[i]) // 100 + 3 * rec) % len(WINDOWS)]
            body = ([] if w is None else list(w)) + [eot]
            if w is None:
                ns[i] = 0.9
            toks[i, :len(body)] = body
            lens[i] = len(body)
            lp[i, :len(body)] = -5.0 if w is None or ((rec, int(seek[i])) in self.hot and t < 0.6) else -0.1
        return B.TranscribeResult(toks, lens, lp, ns, eot)


RECS = (70.0, 33.21, 0.0, 95.5)
CLIPS = [[1.0, 7.0, 7.0, 7.0, 12.0, 50.0, 55.5], "0,3", [], [20.0, 20.5, 21.0, 60.0, 94.0, 200.0]]


def _run_fake(ctx=None, seconds=RECS, **extra):
    ctx = ctx or VadCtx()
    out = B.transcribe_long(ctx, [_rec(s) for s in seconds], **_kw(vocab_size=1 << 16, **extra))   # (timestamp ids need 2 bytes)
    return out, ctx.calls


def test_defaults_spelled_out_make_the_same_calls():
    base_out, base_calls = _run_fake()
    out, calls = _run_fake(vad=None, parallel_clips=None)
    assert calls == base_calls and out == base_out
    assert not any(c[0] == "vad_energy" for c in calls)
    assert all("clip" not in w and "round" not in w for o in out for w in o["windows"])
    assert all("vad_clips" not in o for o in out)
    out, calls = _run_fake(vad=False)
    assert calls == base_calls and out == base_out


def _bursty(n, spans):
    y = np.zeros(n, np.float32)
    for a, b in spans:
        y[a:b] = 5.0
    return y


def test_vad_makes_one_energy_call_and_then_the_calls_of_its_clips():
    content = [int(round(16000 * s)) // 160 for s in RECS]
    tracks = [_bursty(content[0], [(300, 900), (1500, 1600), (4000, 6900)]), np.full(content[1], 1.0, np.float32),
              np.zeros(0, np.float32), _bursty(content[3], [(100, 110), (5000, 9500)])]
    out, calls = _run_fake(VadCtx(tracks), vad=True)
    segs = [V.segments_ref(t)[0] for t in tracks]
    clips = [V.clips_ref(s) for s in segs]
    assert segs[0] == [(280, 920), (1480, 1620), (3980, 6920)] and clips[0] == [(280, 1620), (3980, 6920)]
    assert clips[1] == [(0, content[1])] and clips[2] == [] and clips[3] == [(4980, 9520)]
    assert [o["vad_segments"] for o in out] == segs and [o["vad_clips"] for o in out] == clips
    where = [i for i, c in enumerate(calls) if c[0] == "vad_energy"]
    assert where == [2] and calls[1][0] == "logmel_long"
    T = [c + 3000 for c in content]
    assert calls[2] == ("vad_energy", [int(x) for x in np.cumsum([0] + [80 * t for t in T])[:-1]], T, content, [2, 62], 5, True,
                        False)
    times = [[v / 100.0 for ab in cl for v in ab] if cl else [0.0, 0.0] for cl in clips]
    want, want_calls = _run_fake(clip_timestamps=times)
    assert calls[:2] + calls[3:] == want_calls
    for o, w in zip(out, want):
        assert {k: v for k, v in o.items() if not k.startswith("vad_")} == w
    assert all(w["clip"] in (0, 1) for o in out for w in o["windows"]) and out[2]["windows"] == []
    # the overrides reach the calls
    out2, calls2 = _run_fake(VadCtx(tracks), vad=dict(band=(0, 80), smooth=11, params=dict(speech_pad=0), max_frames=100))
    assert calls2[2][4:6] == ([0, 80], 11)
    assert out2[0]["vad_clips"] == out2[0]["vad_segments"] == [(300, 900), (1500, 1600), (4000, 6900)]


def _without_round(out):
    return [dict(o, windows=[{k: v for k, v in w.items() if k != "round"} for w in o["windows"]]) for o in out]


@pytest.mark.parametrize("n_lanes", [1, 2, 3, 64, True])
def test_parallel_clips_equal_the_sequential_clip_run(n_lanes):
    seq, seq_calls = _run_fake(clip_timestamps=CLIPS, temperatures=(0.0,))
    assert sum(len(o["windows"]) for o in seq) > 12 and any(len(o["windows"]) > 4 for o in seq)
    par, calls = _run_fake(clip_timestamps=CLIPS, temperatures=(0.0,), parallel_clips=n_lanes)
    assert _without_round(par) == seq
    n = 56 if n_lanes is True else n_lanes
    rows = [len(c[3]) for c in calls if c[0] == "transcribe_mel"]
    n_clips = sum(len(B.seek_clips(t, int(round(16000 * s)) // 160)) for t, s in zip(B.clip_times(CLIPS, len(RECS)), RECS))
    assert n_clips == 7 and max(rows) == min(n, n_clips)
    if n >= n_clips:   # as many rounds as the longest lane has windows: fewer than the sequential run's
        longest = max(sum(w["clip"] == c for w in o["windows"]) for o in par for c in {w["clip"] for w in o["windows"]})
        assert len(rows) == longest < len([c for c in seq_calls if c[0] == "transcribe_mel"])
    for o in par:
        per_clip = {}
        for w in o["windows"]:
            per_clip.setdefault(w["clip"], []).append(w)
        assert list(per_clip) == sorted(per_clip)                      # (clip, decode order)
        for ws in per_clip.values():
            assert all(a["seek"] < b["seek"] and a["round"] < b["round"] for a, b in zip(ws, ws[1:]))
        assert [s["id"] for s in o["segments"]] == list(range(len(o["segments"])))
    if n >= n_clips:   # every lane is in every round until it ends: its k-th window is in round k
        assert all(w["round"] == k for o in par for c in {w["clip"] for w in o["windows"]}
                   for k, w in enumerate([w for w in o["windows"] if w["clip"] == c]))


def test_parallel_rows_carry_the_lane_sample_id():
    ids_rec = [7, 300, 65535, 0]
    par, calls = _run_fake(clip_timestamps=CLIPS, temperatures=(0.0,), parallel_clips=3, recording_ids=ids_rec)
    bases = [int(x) for x in np.cumsum([0] + [80 * ((int(round(16000 * s)) + 480000) // 160) for s in RECS])[:-1]]
    seen = {}
    for c in calls:
        if c[0] != "transcribe_mel":
            continue
        for base, seek, sid in zip(c[1], c[3], dict(c[7])["sample_ids"]):
            seen[(bases.index(base), seek)] = sid
    n = 0
    for r, o in enumerate(par):
        count = {}
        for w in o["windows"]:
            k = count.get(w["clip"], 0)
            count[w["clip"]] = k + 1
            assert seen[(r, w["seek"])] == ((((w["clip"] << 4) | min(k, 15)) & 0xFFFF) << 16) | ids_rec[r]
            n += 1
    assert n == len(seen) > 12
    assert {w["clip"] for w in par[0]["windows"]} == {0, 2, 3}   # the empty clip 1 keeps its number


def test_a_parallel_lane_equals_its_clip_alone_under_fallback():
    """With the fallback temperatures a lane's rows differ from the sequential run's in their sample ids only -- and a
    lane's ids are a function of (clip, window within the clip, recording id): the lane alone, its number kept by empty
    clips in front, gives the same records."""
    hot = {(0, 4200), (3, 3300), (3, 9400)}
    par, _ = _run_fake(VadCtx(hot=hot), clip_timestamps=CLIPS, parallel_clips=4)
    assert any(len(w["temperatures"]) > 1 for o in par for w in o["windows"])
    times = B.clip_times(CLIPS, len(RECS))
    for r, sec in enumerate(RECS):
        for a, b, k in B.seek_clips(times[r], int(round(16000 * sec)) // 160):
            alone_times = [[0.0, 0.0] if q != r else [0.0, 0.0] * k + [a / 100.0, b / 100.0] for q in range(len(RECS))]
            alone, _ = _run_fake(VadCtx(hot=hot), clip_timestamps=alone_times, parallel_clips=4)
            mine = [w for w in par[r]["windows"] if w["clip"] == k]
            assert [{q: v for q, v in w.items() if q != "round"} for w in alone[r]["windows"]] == \
                   [{q: v for q, v in w.items() if q != "round"} for w in mine]
            seeks = {w["seek"] for w in mine}
            strip = lambda sg: {q: v for q, v in sg.items() if q != "id"}   # noqa: E731
            assert [strip(s) for s in alone[r]["segments"]] == [strip(s) for s in par[r]["segments"] if s["seek"] in seeks]


def test_parallel_clips_without_clips_is_one_lane_per_recording():
    seq, _ = _run_fake(temperatures=(0.0,))
    par, _ = _run_fake(temperatures=(0.0,), parallel_clips=2)
    assert [dict(o, windows=[{k: v for k, v in w.items() if k not in ("round", "clip")} for w in o["windows"]]) for o in par] == seq
    assert all(w["clip"] == 0 for o in par for w in o["windows"])


def test_vad_and_parallel_clips_together():
    content = [int(round(16000 * s)) // 160 for s in RECS]
    tracks = [_bursty(content[0], [(300, 900), (4000, 6900)]), np.full(content[1], 1.0, np.float32),
              np.zeros(0, np.float32), _bursty(content[3], [(100, 1100), (5000, 9500)])]
    seq, _ = _run_fake(VadCtx(tracks), vad=True, temperatures=(0.0,))
    par, calls = _run_fake(VadCtx(tracks), vad=True, temperatures=(0.0,), parallel_clips=True)
    assert _without_round(par) == seq
    assert [len(o["vad_clips"]) for o in par] == [2, 1, 0, 2]
    assert len(next(c for c in calls if c[0] == "transcribe_mel")[3]) == 5


def test_value_errors(vocab):  # noqa: F811
    for extra in (dict(vad=True, clip_timestamps=[0.0, 5.0]), dict(vad={}, clip_timestamps=""), dict(vad=dict(bands=(0, 1))),
                  dict(parallel_clips=2, condition_on_previous_text=True),
                  dict(parallel_clips=2, hallucination_silence_threshold=2.0, word_timestamps=True, vocab=vocab, no_timestamps=EOT + 7),
                  dict(parallel_clips=0), dict(parallel_clips=-3), dict(parallel_clips=False)):
        ctx = VadCtx([np.zeros(7000 // 1, np.float32)])
        with pytest.raises(ValueError):
            B.transcribe_long(ctx, [_rec(70.0)], **_kw(**extra))
        assert not any(c[0] in ("logmel_long", "transcribe_mel") for c in ctx.calls), extra


# ---------------------------------------------------------------- the reference input
@pytest.fixture(scope="module")
def reference():
    """The f64 long log-mel of the burst recording and of 10 s of 0.05-rms noise."""
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    noise = (0.05 * np.random.default_rng(1).standard_normal(160000)).astype(np.float32)
    return long_log_mel_np(V.bursts(), m80), long_log_mel_np(noise, m80)


def threshold_distance(y, p=None):
    """The smallest |y[t] - threshold| over both thresholds."""
    _, _, on, off = V.thresholds_ref(y, p)
    y = np.asarray(y, dtype=np.float64)
    return float(min(np.abs(y - on).min(), np.abs(y - off).min()))


def energy_tolerance(n_band, smooth, e):
    """The GPU tests' gate on wm_vad_energy: every one of the n_band + smooth f32 additions and the few libm calls costs
    at most about an ulp of a partial result."""
    return 2.0 ** -23 * (n_band + smooth + 16) * max(1.0, float(np.abs(e).max()))


def test_reference_bursts_give_the_three_segments(reference):
    """Measured on the f64 restatement: at smooth 5 the closest frame lies 0.114 from a threshold, at smooth 11 0.025; the
    energy tolerance is 7.1e-5 and 7.5e-5."""
    mel, _ = reference
    n = mel.shape[1] - 3000
    assert n == 4000
    for smooth, least in ((5, 0.1), (11, 0.02)):
        e, y = V.energy_ref(mel, n, 0, 80, smooth)
        d = threshold_distance(y.astype(np.float32))
        tol = energy_tolerance(80, smooth, e)
        print("smooth %d: distance %.4f, tolerance %.3g" % (smooth, d, tol))
        assert d >= least and d >= 100 * tol   # the precondition of every test that compares decisions
        assert V.segments_ref(y.astype(np.float32))[0] == V.BURST_SEGMENTS
        assert B.vad_segments(y.astype(np.float32)) == V.BURST_SEGMENTS
    assert B.vad_clips(V.BURST_SEGMENTS) == [(180, 1622), (2980, 3822)]


def test_reference_noise_alone_fires_the_flat_rule(reference):
    _, mel = reference
    n = mel.shape[1] - 3000
    for band in ((0, 80), B.vad_band(80)):
        _, y = V.energy_ref(mel, n, band[0], band[1], 5)
        got, stats = B.vad_segments(y.astype(np.float32), stats=True)
        assert got == [(0, n)] and stats[1] - stats[0] < 0.3 and math.isnan(stats[2])
