"""CPU tests of long-form transcription (include/whisper_mi355x.h wm_logmel_long, binding.transcribe_long): a numpy
restatement of openai-whisper's log_mel_spectrogram(audio, padding=480000), checked against the 30 s oracle, and the
per-window rules of openai-whisper transcribe() (binding.should_skip_window, binding.window_segments) on hand-built token
streams.  The rules restated, from whisper/transcribe.py (word_timestamps=False):

    if no_speech_threshold is not None:
        should_skip = result.no_speech_prob > no_speech_threshold
        if logprob_threshold is not None and result.avg_logprob > logprob_threshold:
            should_skip = False
        if should_skip:
            seek += segment_size
            continue
    timestamp_tokens = tokens.ge(tokenizer.timestamp_begin)
    single_timestamp_ending = timestamp_tokens[-2:].tolist() == [False, True]
    consecutive = torch.where(timestamp_tokens[:-1] & timestamp_tokens[1:])[0] + 1
    if len(consecutive) > 0:
        slices = consecutive.tolist()
        if single_timestamp_ending:
            slices.append(len(tokens))
        last_slice = 0
        for current_slice in slices:
            sliced_tokens = tokens[last_slice:current_slice]
            start = time_offset + (sliced_tokens[0] - timestamp_begin) * time_precision
            end = time_offset + (sliced_tokens[-1] - timestamp_begin) * time_precision
            current_segments.append(new_segment(start, end, sliced_tokens))
            last_slice = current_slice
        if single_timestamp_ending:
            seek += segment_size
        else:
            seek += (tokens[last_slice - 1] - timestamp_begin) * input_stride
    else:
        duration = segment_duration
        timestamps = tokens[timestamp_tokens.nonzero().flatten()]
        if len(timestamps) > 0 and timestamps[-1] != timestamp_begin:
            duration = (timestamps[-1] - timestamp_begin) * time_precision
        current_segments.append(new_segment(time_offset, time_offset + duration, tokens))
        seek += segment_size
    for segment in current_segments:
        if segment["start"] == segment["end"] or segment["text"].strip() == "":
            segment["text"] = ""; segment["tokens"] = []

time_offset = seek * 0.01, segment_duration = segment_size * 0.01, time_precision = 0.02, input_stride = 2; a segment's
"seek" is the window's first frame."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import logmel_np as L

B = importlib.import_module("openai_whisper_coreml_amd.binding")

N_SAMPLES, HOP, N_FFT = 480000, 160, 400


def long_log_mel_np(x, filt):
    """openai-whisper log_mel_spectrogram(x, padding=480000) in f64: x (any length, any float/int16 dtype already scaled)
    followed by 480000 zeros, torch.stft(n_fft=400, hop=160, periodic Hann, center=True, pad_mode="reflect"), the last
    frame dropped, |.|^2, mel (dense, ascending k, the f32 filter widened), log10(max(., 1e-10)), max(., max - 8),
    (. + 4) / 4.  Returns [n_mels][(len + 480000) // 160]."""
    sig = np.concatenate([np.asarray(x, dtype=np.float64), np.zeros(N_SAMPLES)])
    a = np.pad(sig, 200, mode="reflect")
    T = sig.size // HOP
    idx = (np.arange(T) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(a[idx] * L.hann_periodic()[None, :], axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    f64 = np.asarray(filt, dtype=np.float64)
    mel = np.zeros((f64.shape[0], T), dtype=np.float64)
    for k in range(201):
        mel += f64[:, k:k + 1] * power[None, :, k]
    mel = np.log10(np.where(mel > 1e-10, mel, 1e-10))
    return (np.maximum(mel, mel.max() - 8.0) + 4.0) / 4.0


def loud_start(n, seed=0):
    """Noise with a loud tone in its first second: the recording's maximum lies in the first frames."""
    rng = np.random.default_rng(seed)
    x = np.clip(0.05 * rng.standard_normal(n), -1, 1)
    m = min(n, 16000)
    x[:m] += 0.8 * np.sin(2 * np.pi * 440 * np.arange(m) / 16000)
    return x.astype(np.float32)


def test_long_log_mel_restatement_matches_the_30s_oracle():
    """Frames [0, 2999) of a 30 s recording see the same samples in both paddings (frame 2999 reaches past sample 480000:
    a reflection in the 30 s chunk, a zero in the long signal); with the maximum there, the values agree."""
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    x = loud_start(N_SAMPLES)
    want = L.log_mel(x, m80)
    got = long_log_mel_np(x, m80)
    assert got.shape == (80, 6000)
    assert np.argmax(want.max(axis=0)) < 2999
    assert np.abs(got[:, :2999] - want[:, :2999]).max() <= 1e-12


def test_long_log_mel_of_silence_and_frame_counts():
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    for n in (0, 1, 159, 160, 4000):
        got = long_log_mel_np(np.zeros(n), m80)
        assert got.shape == (80, (n + N_SAMPLES) // 160)
        assert np.all(got == -1.5)      # log10(1e-10) = -10, clamp at -18, (-10 + 4) / 4


TB, EOT = 100, 50                       # timestamp_begin and eot of the hand-built streams
RES = dict(temperature=0.2, avg_logprob=-0.3, compression_ratio=1.1, no_speech_prob=0.01)


class FakeVocab:
    WORDS = {10: "a", 11: "b", 12: "c", 13: " ", 14: "d"}

    def decode(self, ids):
        return "".join(self.WORDS.get(int(i), "") for i in ids)


def _seg(r):
    return [(s["seek"], s["start"], s["end"], s["tokens"]) for s in r]


def test_consecutive_pairs_without_a_single_timestamp_ending():
    toks = [TB, 10, 11, TB + 5, TB + 5, 12, TB + 9, TB + 9, 13]
    segs, seek = B.window_segments(toks, 300, 3000, TB, EOT, RES)
    off = 300 * 0.01
    assert _seg(segs) == [(300, off + 0 * 0.02, off + 5 * 0.02, [TB, 10, 11, TB + 5]),
                          (300, off + 5 * 0.02, off + 9 * 0.02, [TB + 5, 12, TB + 9])]
    assert seek == 300 + 9 * 2          # the unfinished tail [TB + 9, 13] is dropped: seek to the last timestamp
    for s in segs:
        assert (s["temperature"], s["avg_logprob"], s["compression_ratio"], s["no_speech_prob"]) == (0.2, -0.3, 1.1, 0.01)


def test_consecutive_pairs_with_a_single_timestamp_ending():
    toks = [TB, 10, TB + 5, TB + 5, 11, TB + 8]
    segs, seek = B.window_segments(toks, 0, 3000, TB, EOT, RES)
    assert _seg(segs) == [(0, 0.0, 5 * 0.02, [TB, 10, TB + 5]), (0, 5 * 0.02, 8 * 0.02, [TB + 5, 11, TB + 8])]
    assert seek == 3000


def test_no_pair_with_a_final_timestamp():
    segs, seek = B.window_segments([TB, 10, 11, TB + 7], 1000, 3000, TB, EOT, RES)
    assert _seg(segs) == [(1000, 10.0, 10.0 + 7 * 0.02, [TB, 10, 11, TB + 7])]
    assert seek == 4000


def test_no_pair_without_a_timestamp():
    segs, seek = B.window_segments([10, 11], 1000, 3000, TB, EOT, RES)
    assert _seg(segs) == [(1000, 10.0, 10.0 + 3000 * 0.01, [10, 11])]
    assert seek == 4000


def test_final_timestamp_equal_to_timestamp_begin_keeps_the_window_duration():
    segs, seek = B.window_segments([TB, 10, 11, TB], 0, 3000, TB, EOT, RES)
    assert _seg(segs) == [(0, 0.0, 30.0, [TB, 10, 11, TB])]
    assert seek == 3000


def test_silence_skip_and_its_logprob_override():
    assert B.should_skip_window(0.7, -2.0, 0.6, -1.0)
    assert not B.should_skip_window(0.7, -0.5, 0.6, -1.0)       # avg_logprob > threshold: decoded anyway
    assert not B.should_skip_window(0.5, -2.0, 0.6, -1.0)
    assert B.should_skip_window(0.7, -0.5, 0.6, None)            # no logprob threshold: no override
    assert not B.should_skip_window(0.9, -9.0, None, -1.0)


def test_clearing_instantaneous_and_textless_segments():
    # pairs at 0|1 and 1|2 give the instantaneous segments [TB] and [TB + 3]; the third one has text
    toks = [TB, TB + 3, TB + 3, 10, TB + 6]
    segs, seek = B.window_segments(toks, 0, 3000, TB, EOT, RES)
    assert _seg(segs) == [(0, 0.0, 0.0, []), (0, 3 * 0.02, 3 * 0.02, []), (0, 3 * 0.02, 6 * 0.02, [TB + 3, 10, TB + 6])]
    assert seek == 3000
    # no token below eot: text-less without a Vocab
    segs, _ = B.window_segments([TB + 5], 0, 3000, TB, EOT, RES)
    assert _seg(segs) == [(0, 0.0, 5 * 0.02, [])]
    segs, _ = B.window_segments([], 0, 3000, TB, EOT, RES)
    assert _seg(segs) == [(0, 0.0, 30.0, [])]
    # with a Vocab, text-less is blank decoded text
    segs, _ = B.window_segments([TB, 13, TB + 4], 0, 3000, TB, EOT, RES, vocab=FakeVocab())
    assert segs[0]["tokens"] == [] and segs[0]["text"] == ""
    segs, _ = B.window_segments([TB, 13, 14, TB + 4], 0, 3000, TB, EOT, RES, vocab=FakeVocab())
    assert segs[0]["tokens"] == [TB, 13, 14, TB + 4] and segs[0]["text"] == " d"


def test_last_short_window():
    segs, seek = B.window_segments([10, 11], 9000, 1234, TB, EOT, RES)
    assert _seg(segs) == [(9000, 90.0, 90.0 + 1234 * 0.01, [10, 11])]
    assert seek == 9000 + 1234
    segs, seek = B.window_segments([TB, 10, TB + 3, TB + 3, 11], 9000, 1234, TB, EOT, RES)
    assert _seg(segs) == [(9000, 90.0, 90.0 + 3 * 0.02, [TB, 10, TB + 3])]
    assert seek == 9000 + 3 * 2


def test_pack_recordings_dtypes_and_offsets():
    a = np.array([1, -2, 3], dtype=np.int16)
    b = np.array([0.5, 0.25], dtype=np.float32)
    pcm, offs = B._pack_recordings([a, a])
    assert pcm.dtype == np.int16 and list(offs) == [0, 3, 6]
    pcm, offs = B._pack_recordings([a, np.zeros(0, np.float32), b])
    assert pcm.dtype == np.float32 and list(offs) == [0, 3, 3, 5]
    assert np.array_equal(pcm, np.array([1 / 32768, -2 / 32768, 3 / 32768, 0.5, 0.25], dtype=np.float32))


def test_fallback_decode_is_the_rule_of_transcribe_with_fallback():
    """fallback_decode over a scripted decode: step k re-decodes exactly the rows that failed step k - 1."""
    calls = []

    def decode(todo, t, sd):
        calls.append((list(todo), t, sd))
        n = len(todo)
        toks = np.full((n, 4), EOT, dtype=np.int32)
        toks[:, 0] = 7
        lens = np.full(n, 2, dtype=np.int32)
        # row 1 stays bad until T = 0.4; the others are good at once
        lp = np.array([[-2.0 if (b == 1 and t < 0.4) else -0.1, -0.1, 0, 0] for b in todo], dtype=np.float32)
        return B.TranscribeResult(toks, lens, lp, np.zeros(n, np.float32), EOT)

    out = B.fallback_decode(decode, 3, 1024, 4, EOT, seed=5, compression_ratio_threshold=None)
    assert [c[0] for c in calls] == [[0, 1, 2], [1], [1]]
    assert [c[1] for c in calls] == [0.0, 0.2, 0.4] and [c[2] for c in calls] == [5, 6, 7]
    assert list(out["temperature"]) == [0.0, 0.4, 0.0] and not out["needs_fallback"].any()
