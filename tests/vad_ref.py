"""f64 numpy restatements of the speech-activity path: wm_vad_energy's definition, wm_vad_segments' rule and vad_clips,
written from include/whisper_mi355x.h and not from the library's code.  Shared by tests/test_vad_cpu.py and
tests/test_vad_gpu.py."""
import math

import numpy as np

DEFAULTS = dict(q_floor=0.10, q_peak=0.95, min_range=0.6, on_frac=0.5, off_frac=0.35, min_speech=25, min_silence=50,
                speech_pad=40)
FLOAT_FIELDS = ("q_floor", "q_peak", "min_range", "on_frac", "off_frac")


def energy_ref(mel, n, lo, hi, smooth):
    """(e, y) f64 [n] of one recording's log-mel block mel [n_mels][T]: e = log10 of the band's mel power + 4 (through
    the same shift by the band's maximum, exact in f64), y = its centred moving average clipped to [0, n)."""
    v = np.asarray(mel, dtype=np.float64)[lo:hi, :n]
    if n == 0:
        return np.zeros(0), np.zeros(0)
    vmax = v.max(axis=0)
    s = np.exp2((v - vmax) * (4.0 * math.log2(10.0))).sum(axis=0)
    e = 4.0 * vmax + np.log10(s)
    h = smooth // 2
    a = np.maximum(np.arange(n) - h, 0)
    z = np.minimum(np.arange(n) + h, n - 1)
    y = np.array([e[a[t]:z[t] + 1].sum() for t in range(n)]) / (z - a + 1)
    return e, y


def params_f32(p=None):
    """The parameters as the C struct holds them: the float fields rounded to f32, then read back as doubles."""
    q = dict(DEFAULTS)
    q.update(p or {})
    for k in FLOAT_FIELDS:
        q[k] = float(np.float32(q[k]))
    return q


def thresholds_ref(y, p=None):
    """(floor, peak, thr_on, thr_off) in double; the thresholds are NaN under the flat rule; None for n = 0."""
    q = params_f32(p)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    n = y.size
    if n == 0:
        return None
    s = np.sort(y)
    floor, peak = s[int(q["q_floor"] * (n - 1))], s[int(q["q_peak"] * (n - 1))]
    if peak - floor < q["min_range"]:
        return floor, peak, math.nan, math.nan
    return floor, peak, floor + q["on_frac"] * (peak - floor), floor + q["off_frac"] * (peak - floor)


def segments_ref(y, p=None):
    """wm_vad_segments: [(start, end)] and the four stats as f32 (NaN where undefined)."""
    q = params_f32(p)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    n = y.size
    nan4 = tuple([np.float32(np.nan)] * 4)
    if n == 0:
        return [], nan4
    floor, peak, on, off = thresholds_ref(y, p)
    stats = tuple(np.float32(x) for x in (floor, peak, on, off))
    if math.isnan(on):
        return [(0, n)], stats
    raw = []
    trig, pend, start = False, -1, 0
    for t in range(n):
        if y[t] >= on:
            pend = -1
        if not trig and y[t] >= on:
            trig, start = True, t
        elif trig and y[t] < off:
            if pend < 0:
                pend = t
            if t + 1 - pend >= q["min_silence"]:
                if pend - start >= q["min_speech"]:
                    raw.append((start, pend))
                trig, pend = False, -1
    if trig and n - start >= q["min_speech"]:
        raw.append((start, n))
    out = []
    for a, b in raw:
        a, b = max(0, a - q["speech_pad"] // 2), min(n, b + q["speech_pad"] // 2)   # speech_pad frames over both sides
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out, stats


def clips_ref(segments, max_frames=3000):
    clips = []
    for a, b in segments:
        if clips and b - clips[-1][0] <= max_frames:
            clips[-1] = (clips[-1][0], b)
        else:
            clips.append((a, b))
    return clips


def slaney_centres(n_mels):
    """Centre frequencies (Hz) of the n_mels Slaney-scale filters between 0 and 8000 Hz (librosa.filters.mel)."""
    def hz_to_mel(f):
        return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0) if f >= 1000.0 else f / (200.0 / 3.0)

    def mel_to_hz(m):
        return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0)) if m >= 15.0 else (200.0 / 3.0) * m
    pts = np.linspace(hz_to_mel(0.0), hz_to_mel(8000.0), n_mels + 2)
    return [mel_to_hz(m) for m in pts[1:-1]]


def bursts(seconds=40.0, spans=((2, 5), (5.3, 9), (15, 16), (20, 20.1), (30, 38)), noise=0.001, seed=0):
    """The reference input: `seconds` of `noise`-rms Gaussian noise with three-tone bursts over the given spans (seconds):
    0.1 (sin 220 + sin 880 + sin 2200 Hz) -- amplitude 0.3 -- under a 4 Hz tremolo 0.6 + 0.4 sin(2 pi 4 u), u the time
    since the burst began.  f32 at 16 kHz."""
    n = int(round(seconds * 16000))
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = noise * np.random.default_rng(seed).standard_normal(n)
    for a, b in spans:
        i0, i1 = int(round(a * 16000)), int(round(b * 16000))
        tt, u = t[i0:i1], np.arange(i1 - i0) / 16000.0
        tone = 0.1 * (np.sin(2 * np.pi * 220 * tt) + np.sin(2 * np.pi * 880 * tt) + np.sin(2 * np.pi * 2200 * tt))
        x[i0:i1] += tone * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * u))
    return x.astype(np.float32)


BURST_SEGMENTS = [(180, 921), (1480, 1622), (2980, 3822)]
