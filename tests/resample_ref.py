"""f64 restatement of the library's resampler (include/whisper_mi355x.h): numpy only.

    g = gcd(sr, 16000), L = 16000 / g, M = sr / g, mx = max(L, M), K = 32 mx
    c = 0.9 / (2 mx),  h[j] = L 2c sinc(2c j) I0(9.62 sqrt(1 - (j / K)^2)) / I0(9.62),  j = -K .. K
    y[n] = sum_k m[k] h[n M - k L],  n < ceil(N L / M),  m zero outside [0, N)

which is scipy.signal.resample_poly(m, L, M, window=h / L) (tests/test_resample_cpu.py pins that)."""
import math

import numpy as np

TARGET = 16000
ZEROS, ROLLOFF, BETA = 32, 0.9, 9.62
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def params(sr):
    g = math.gcd(int(sr), TARGET)
    L, M = TARGET // g, int(sr) // g
    return L, M, ZEROS * max(L, M)


def supported(sr):
    return 4000 <= sr <= 192000 and params(sr)[0] <= 640


def i0(x):
    """Modified Bessel function of the first kind, order 0: the power series (all terms positive)."""
    x = np.asarray(x, dtype=np.float64)
    q = x * x / 4.0
    term = np.ones_like(x)
    total = np.ones_like(x)
    for k in range(1, 200):
        term = term * q / (k * k)
        total = total + term
        if np.all(term < 1e-20 * total):
            break
    return total


def prototype(sr):
    """h f64 [2K + 1] (index j + K), L, M, K."""
    L, M, K = params(sr)
    j = np.arange(-K, K + 1, dtype=np.float64)
    c = ROLLOFF / (2.0 * max(L, M))
    w = i0(BETA * np.sqrt(np.maximum(1.0 - (j / K) ** 2, 0.0))) / i0(BETA)
    return L * 2.0 * c * np.sinc(2.0 * c * j) * w, L, M, K


def taps(sr):
    L, M, K = params(sr)
    return -(-(2 * K + 1) // L)


def out_len(n, sr):
    L, M, _ = params(sr)
    return -(-n * L // M)


def downmix(x):
    """[n] or [n][C] int16 / float32 -> mono f32 by the library's rule: the f32 sum in channel order times f32(1 / C);
    int16 samples are s / 32768."""
    x = np.asarray(x)
    f = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)
    if f.ndim == 1:
        return f
    if f.shape[1] == 1:
        return f[:, 0].copy()
    s = f[:, 0].copy()
    for c in range(1, f.shape[1]):
        s = s + f[:, c]
    return s * np.float32(1.0 / f.shape[1])


def resample(m, sr, h=None):
    """The direct sum in f64.  m: mono samples; returns y f64 [ceil(N L / M)]."""
    m = np.asarray(m, dtype=np.float64)
    if h is None:
        h = prototype(sr)[0]
    L, M, K = params(sr)
    N = len(m)
    n_out = out_len(N, sr)
    y = np.zeros(n_out, dtype=np.float64)
    T = -(-(2 * K + 1) // L)
    n = np.arange(n_out, dtype=np.int64)
    kf = -((K - n * M) // L)              # ceil((n M - K) / L)
    for u in range(T):
        k = kf + u
        j = n * M - k * L
        ok = (k >= 0) & (k < N) & (j >= -K)
        y[ok] += m[k[ok]] * h[j[ok] + K]
    return y
