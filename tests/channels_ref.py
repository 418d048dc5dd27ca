"""f64 restatement of the multichannel front (include/whisper_mi355x.h): numpy only.

The mix of wm_resample_16k_mix: per frame sum_c w[c] x[c] in f64 (x = s / 32768 for int16), then resample_ref.resample.
The library's own mixed sample is m = w[0] x[0] rounded to f32, then m = fmaf(w[c], x[c], m) in channel order: C roundings.

The activity of wm_channel_activity: per 160-sample frame the f64 sum of |y| (the last frame may be short).  The
library's f32 sum runs in this order, a function of the frame alone (activity_f32 restates it operation for operation):

    p[j] = ((|y[j]| + |y[16 + j]|) + ...) + |y[144 + j]|      j = 0 .. 15: ten terms, ascending; a term past the end is +0
    q[j] = p[j] + p[j + 8],  r[j] = q[j] + q[j + 4],  t[j] = r[j] + r[j + 2],  act = t[0] + t[1]
"""
import numpy as np

import resample_ref

HOP = 160


def as_f64(x):
    """[n] or [n][C] int16 / float32 -> f64 [n][C]; int16 samples are s / 32768"""
    x = np.asarray(x)
    f = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    return f[:, None] if f.ndim == 1 else f


def mix(x, w):
    """the mixed mono signal of one row, f64 [n]"""
    return as_f64(x) @ np.asarray(w, dtype=np.float64)


def mix_scale(x, w):
    """A of the error gate: max_k sum_c |w_c| |x_c[k]| (0 for an empty recording)"""
    f = np.abs(as_f64(x)) @ np.abs(np.asarray(w, dtype=np.float64))
    return float(f.max()) if f.size else 0.0


def resample_mix(x, sr, w, h=None):
    """signal (recording x at sr Hz, row w) in f64; at 16000 Hz the mix itself"""
    m = mix(x, w)
    return m if sr == resample_ref.TARGET else resample_ref.resample(m, sr, h)


def activity(y):
    """f64 [ceil(N / 160)]: the sum of |y| per frame"""
    y = np.abs(np.asarray(y, dtype=np.float64))
    n = -(-len(y) // HOP)
    pad = np.zeros(n * HOP, dtype=np.float64)
    pad[:len(y)] = y
    return pad.reshape(n, HOP).sum(axis=1)


def activity_f32(y):
    """the library's f32 sum in the library's order"""
    y = np.abs(np.asarray(y, dtype=np.float32))
    n = -(-len(y) // HOP)
    pad = np.zeros(n * HOP, dtype=np.float32)
    pad[:len(y)] = y
    t = pad.reshape(n, HOP // 16, 16)
    p = t[:, 0, :].copy()
    for i in range(1, HOP // 16):
        p = p + t[:, i, :]
    q = p[:, :8] + p[:, 8:]
    r = q[:, :4] + q[:, 4:]
    s = r[:, :2] + r[:, 2:]
    return s[:, 0] + s[:, 1]
