"""f64 restatement of a live stream's frames (include/whisper_mi355x.h, wm_streams_*), on the arithmetic of
test_longform_cpu.long_log_mel_np: frame t of a stream that has received the samples x reads [160 t - 200, 160 t + 200) -- an
index n < 0 reads sample -n, a sample that has not arrived reads 0 -- and gives log10(max(mel, 1e-10)) per mel row; a window
of frames is normalised by the maximum over exactly its frames."""
import numpy as np

from oracle import logmel_np as L

HOP, N_FFT = 160, 400


def counts_brute(n, capacity):
    """(final F, avail A, first kept K) of a stream of n samples, frame by frame from the definition."""
    def reads(t):
        return np.abs(np.arange(HOP * t - 200, HOP * t + 200))
    final = avail = 0
    t = 0
    while True:
        r = reads(t)
        if n > 0 and r.min() < n:
            avail = t + 1
        else:
            break
        t += 1
    prefix = True
    for t in range(avail):
        if prefix and reads(t).max() < n:
            final = t + 1
        else:
            prefix = False
    return final, avail, max(0, avail - capacity)


def counts(n, capacity):
    """the closed forms of the header"""
    final = 0 if n < 201 else (n - 200) // HOP + 1
    avail = 0 if n == 0 else (n + 199) // HOP + 1
    return final, avail, max(0, avail - capacity)


def raw_frames(x, filt, n_frames=None, from_start=True):
    """Raw frames [0, n_frames) (default: all avail frames) of a stream whose samples so far are x (already scaled), f64
    [n_mels][n_frames].  from_start=False: silence came before x, a whole number of hops of it, and frame 0 is
    the frame centred at x[0] -- it reads 200 samples of that silence, no reflection (a stream placed past its start)."""
    x = np.asarray(x, dtype=np.float64)
    if n_frames is None:
        n_frames = counts(x.size, 1 << 60)[1]
    sig = np.concatenate([x, np.zeros(HOP * n_frames + N_FFT + 200)])
    a = np.pad(sig, (200, 0), mode="reflect") if from_start else np.concatenate([np.zeros(200), sig])
    idx = (np.arange(n_frames) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(a[idx] * L.hann_periodic()[None, :], axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    f64 = np.asarray(filt, dtype=np.float64)
    mel = np.zeros((f64.shape[0], n_frames), dtype=np.float64)
    for k in range(201):
        mel += f64[:, k:k + 1] * power[None, :, k]
    return np.log10(np.where(mel > 1e-10, mel, 1e-10))


def window(raw, first, n):
    """frames [first, first + n) of raw, normalised as a recording that is the window"""
    w = raw[:, first:first + n]
    return (np.maximum(w, w.max() - 8.0) + 4.0) / 4.0
