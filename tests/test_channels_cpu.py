"""CPU tests of the multichannel front: the f64 restatement tests/channels_ref.py, the host rule
binding.speaker_by_channel, binding.channel_rows, and binding.transcribe_long(channels=...) on a scripted fake context in the
style of tests/test_longform_calls_cpu.py: every Context call is logged with its arguments."""
import copy
import ctypes
import importlib
import json

import numpy as np
import pytest

import channels_ref as cref
import resample_ref as ref
from test_longform_calls_cpu import CONTENT, HOT, LANGS, NO_TEXT, SCRIPT, SKIP, STD, RecCtx, _tracks, canon, make_vocab
from test_longform_words_cpu import LANG_EN, LANG_ZH, NO_TS

B = importlib.import_module("openai_whisper_coreml_amd.binding")


# ---------------------------------------------------------------- the restatement
def test_the_f64_mix_is_the_weighted_sum_and_a_one_hot_row_is_the_channel():
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, size=(700, 3)).astype(np.int16)
    w = np.array([0.25, -1.0, 0.5], np.float32)
    m = cref.mix(x, w)
    assert np.array_equal(m, (0.25 * x[:, 0] - 1.0 * x[:, 1] + 0.5 * x[:, 2]) / 32768.0)      # exact in f64
    assert cref.mix_scale(x, w) == float(np.max((0.25 * np.abs(x[:, 0].astype(np.float64)) + np.abs(x[:, 1].astype(np.float64))
                                                 + 0.5 * np.abs(x[:, 2].astype(np.float64))) / 32768.0))
    for sr in (48000, 44100, 8000):
        one = cref.resample_mix(x, sr, [0, 1, 0])
        assert np.array_equal(one, ref.resample(x[:, 1].astype(np.float64) / 32768.0, sr))
        assert one.shape == (ref.out_len(700, sr),)
    assert np.array_equal(cref.resample_mix(x, 16000, w), m)                                   # the bypass: the mix itself
    assert cref.mix(np.zeros((0, 2), np.float32), [1, 1]).shape == (0,) and cref.mix_scale(np.zeros((0, 2), np.float32), [1, 1]) == 0.0
    mono = rng.uniform(-1, 1, 50).astype(np.float32)
    assert np.array_equal(cref.mix(mono, [2.0]), 2.0 * mono.astype(np.float64))


def test_the_f64_activity_and_the_f32_order():
    rng = np.random.default_rng(2)
    for n in (0, 1, 159, 160, 161, 160 * 7 + 37):
        y = rng.uniform(-1, 1, n).astype(np.float32)
        a = cref.activity(y)
        assert a.shape == (-(-n // 160),) and a.dtype == np.float64
        for f in range(len(a)):   # (numpy's own summation order differs between the two: 160 terms below 1, in f64)
            assert abs(a[f] - np.abs(y[160 * f:160 * (f + 1)].astype(np.float64)).sum()) <= 1e-12
        a32 = cref.activity_f32(y)
        assert a32.dtype == np.float32 and a32.shape == a.shape
        assert np.all(np.abs(a32 - a) <= 160 * 2.0 ** -24 * a)                                  # the library's gate holds for its order
    y = np.ones(400, np.float32)
    y[170] = np.nan
    assert np.isnan(cref.activity(y)[1]) and np.isnan(cref.activity_f32(y)[1])
    assert list(cref.activity(y)[[0, 2]]) == [160.0, 80.0] and list(cref.activity_f32(y)[[0, 2]]) == [160.0, 80.0]
    # the order, element by element, on one frame whose sum depends on it
    z = (np.float32(1.0) + np.arange(160, dtype=np.float32) * np.float32(2.0 ** -20)) * np.float32(1e-3)
    p = [np.float32(0)] * 16
    for j in range(16):
        acc = z[j]
        for i in range(1, 10):
            acc = np.float32(acc + z[16 * i + j])
        p[j] = acc
    q = [np.float32(p[j] + p[j + 8]) for j in range(8)]
    r = [np.float32(q[j] + q[j + 4]) for j in range(4)]
    t = [np.float32(r[j] + r[j + 2]) for j in range(2)]
    assert cref.activity_f32(z)[0] == np.float32(t[0] + t[1])


# ---------------------------------------------------------------- channel_rows, speaker_by_channel
def test_channel_rows():
    assert np.array_equal(B.channel_rows("split", 3), np.eye(3, dtype=np.float32)) and B.channel_rows("split", 3).dtype == np.float32
    m = B.channel_rows("mean", 3)
    assert m.shape == (1, 3) and m.dtype == np.float32 and np.all(m == np.float32(1.0 / 3))
    assert np.array_equal(B.channel_rows(2, 3), np.array([[0, 0, 1]], np.float32))
    assert np.array_equal(B.channel_rows("split", 1), np.ones((1, 1), np.float32))
    for bad in (("left", 2), (2, 2), (-1, 2), (True, 2), (0.0, 2), ("split", 0)):
        with pytest.raises(ValueError):
            B.channel_rows(*bad)


def _act(*levels, frames=400):
    """[C][F]: channel c at level levels[c]"""
    return [np.full(frames, v, np.float32) for v in levels]


def test_speaker_by_channel_cases():
    S = B.speaker_by_channel
    assert S(_act(2.0, 1.0), 0.0, 1.0) == 0 and S(_act(1.0, 2.0), 0.0, 1.0) == 1                 # a clear winner
    assert S(_act(2.0, 1.0), 0.0, 1.0, ratio=2.0) is None                                         # exactly ratio times: strict
    assert S(_act(2.0, 1.0), 0.0, 1.0, ratio=1.9999) == 0
    assert S(_act(1.0, 1.0), 0.0, 1.0) is None and S(_act(1.0, 1.0), 0.0, 1.0, ratio=1) is None   # a tie
    assert S(_act(0.0, 0.0), 0.0, 1.0) is None                                                    # all zero
    assert S(_act(1.0, 0.0), 0.0, 1.0) == 0                                                       # the other silent
    assert S(_act(3.0), 0.0, 1.0) is None and S([], 0.0, 1.0) is None                             # one channel, none
    nan = _act(5.0, 1.0)
    nan[1][50] = np.nan
    assert S(nan, 0.0, 1.0) is None and S(nan, 0.51, 1.0) == 0                                    # NaN inside / outside the span
    # C = 3, the runner-up not adjacent: channel 2 leads, channel 0 follows
    assert S(_act(1.0, 0.1, 1.05), 0.0, 1.0) is None and S(_act(1.0, 0.1, 1.05), 0.0, 1.0, ratio=1.04) == 2
    assert S(_act(1.0, 5.0, 1.0), 0.0, 1.0) == 1
    # the first maximum is `best`: two equal leaders never win
    assert S(_act(2.0, 0.5, 2.0), 0.0, 1.0) is None


def test_speaker_by_channel_spans():
    S = B.speaker_by_channel
    a = [np.zeros(400, np.float32), np.zeros(400, np.float32)]
    a[0][:200] = 1.0      # left speaks in [0, 2) s
    a[1][200:] = 1.0      # right in [2, 4) s
    assert S(a, 0.2, 1.8) == 0 and S(a, 2.2, 3.8) == 1
    assert S(a, -5.0, 1.0) == 0                       # cut at the front: frames [0, 100)
    assert S(a, 3.0, 99.0) == 1                       # cut at the end: frames [300, 400)
    assert S(a, -9.0, 99.0) is None                   # everything: a tie
    assert S(a, 1.0, 1.0) is None                     # empty: [100, 100)
    assert S(a, 2.0, 1.0) is None and S(a, 4.0, 5.0) is None and S(a, -2.0, -1.0) is None
    # floor / ceil: [1.995, 2.001) are the frames [199, 201): one frame each
    assert S(a, 1.995, 2.001) is None and S(a, 1.985, 2.001) == 0 and S(a, 1.995, 2.011) == 1
    # sums in f64: 2^25 + 1 frames' worth of level cannot be told apart in f32
    big = [np.array([2.0 ** 25, 1.0, 1.0], np.float32), np.array([2.0 ** 25, 1.0, 0.0], np.float32)]
    assert S(big, 0.0, 0.03, ratio=1) == 0


def test_speaker_by_channel_ratio_errors():
    for bad in (0.99, 0, -1, float("nan"), float("inf"), None, "1.1", True):
        with pytest.raises(ValueError):
            B.speaker_by_channel(_act(2.0, 1.0), 0.0, 1.0, ratio=bad)


# ---------------------------------------------------------------- transcribe_long on a scripted fake
class ChanCtx(RecCtx):
    """RecCtx plus the two multichannel calls.  activity: the tracks channel_activity hands back (one per signal)."""

    def __init__(self, script, activity=None, **kw):
        super().__init__(script, **kw)
        self.activity = activity

    def resample_16k_mix(self, *a, **kw):
        self._log("resample_16k_mix", a, kw)
        assert kw == dict(device=True)
        n = [-(-len(r) * 16000 // int(sr)) for r, sr in zip(a[0], a[1])]
        per = [n_r for n_r, m in zip(n, a[2]) for _ in range(len(m))]
        return ctypes.c_void_p(8192), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)

    def channel_activity(self, *a, **kw):
        self._log("channel_activity", a, kw)
        assert kw == dict(device=True) and len(self.activity) == len(a[1]) - 1
        return [np.asarray(t, dtype=np.float32) for t in self.activity]

    def set_sequence_bias_tables(self, *a, **kw):
        self._log("set_sequence_bias_tables", a, kw)

    def set_bias_rows(self, *a, **kw):
        self._log("set_bias_rows", a, kw)


RATES = [8000, 44100, 16000]
COUNTS = [2, 1, 2]                                         # channels per recording -> 5 channel-recordings
SECONDS = (70.0, 37.5, 0.01)                               # CONTENT frames, as the calls test's recordings
FLAT_CONTENT = [CONTENT[0], CONTENT[0], CONTENT[1], CONTENT[2], CONTENT[2]]
# keys (recording id, window ordinal): channel-recordings 0 and 1 are recording 0's, 2 is recording 1's, 3 and 4 recording 2's
SPLIT_SCRIPT = {(0, 1): HOT, (0, 2): NO_TEXT, (1, 0): SKIP, (2, 0): SKIP, (2, 1): HOT, (1, 1): HOT}


def _multi():
    return [np.zeros((int(round(8000 * SECONDS[0])), 2), np.int16), np.zeros(int(round(44100 * SECONDS[1])), np.float32),
            np.zeros((160, 2), np.int16)]


def _flat():
    return [np.zeros(c * 160, np.float32) for c in FLAT_CONTENT]


def _j(x):
    return json.loads(json.dumps(canon(x)))


def _run(ctx, recs, **kw):
    return B.transcribe_long(ctx, recs, **kw)


def _split_and_flat(kw_split, kw_flat, script=SPLIT_SCRIPT, **ctx_kw):
    a, b = ChanCtx(script, **ctx_kw), ChanCtx(script, **ctx_kw)
    got = _run(a, _multi(), sample_rates=RATES, channels="split", **kw_split)
    want = _run(b, _flat(), sample_rates=[16000] * 5, **kw_flat)
    return a, got, b, want


def _assert_split_is_flat(a, got, b, want):
    """ONE mix call where the flat run has its resample_16k call; every other call the flat run's, argument for argument"""
    names_a, names_b = [c[0] for c in a.calls], [c[0] for c in b.calls]
    at = names_b.index("resample_16k")
    assert names_a.count("resample_16k_mix") == 1 and names_a.index("resample_16k_mix") == at
    assert "resample_16k" not in names_a and "channel_activity" not in names_a
    assert a.calls[:at] == b.calls[:at] and a.calls[at + 1:] == b.calls[at + 1:]
    assert names_a[at + 1:at + 3] == ["logmel_long_device", "dev_free"]
    mixes = a.calls[at][1][2]
    assert a.calls[at][1][1] == RATES and mixes == [np.eye(C).tolist() for C in COUNTS] and a.calls[at][2] == [["device", True]]
    # the result: per recording its channels' results and the merged segments
    assert len(got) == len(COUNTS) and len(want) == sum(COUNTS)
    i = 0
    for rec, C in zip(got, COUNTS):
        assert sorted(rec) == ["channels", "segments"]
        assert _j(rec["channels"]) == _j(want[i:i + C])
        merged = [dict(sg, channel=c) for c in range(C) for sg in want[i + c]["segments"]]
        merged.sort(key=lambda sg: (sg["start"], sg["channel"]))
        assert _j(rec["segments"]) == _j(merged)
        assert [(sg["start"], sg["channel"]) for sg in rec["segments"]] == sorted((sg["start"], sg["channel"]) for sg in rec["segments"])
        i += C


def test_split_is_one_mix_call_and_the_flat_mono_run():
    a, got, b, want = _split_and_flat(STD, STD)
    _assert_split_is_flat(a, got, b, want)
    # the scripted windows did their work: a fallback, a skip, and segments on both channels of recording 0
    windows = [w for ch in got[0]["channels"] for w in ch["windows"]]
    assert any(len(w["temperatures"]) > 1 for w in windows) and any(w["skipped"] for w in windows)
    assert {sg["channel"] for sg in got[0]["segments"]} == {0, 1} and len(got[0]["segments"]) >= 4
    assert all(sg["channel"] == 0 for sg in got[1]["segments"])
    # a copy: the merged segments are not the channels' own dicts
    got[0]["segments"][0]["start"] = -1.0
    assert all(sg["start"] >= 0 for ch in got[0]["channels"] for sg in ch["segments"])


def test_split_repeats_per_recording_lists_per_channel():
    per_rec = dict(language=[LANG_EN, LANG_ZH, LANG_EN], initial_prompt_tokens=[[3, 4], [], [5]],
                   clip_timestamps=[[0.0, 4.0, 20.0, 75.0], "0,3", []],
                   recording_bias=[dict(bad_words=[[7]]), None, dict(sequence_bias={(8, 9): 1.5})])
    rep = lambda v: [v[r] for r, C in enumerate(COUNTS) for _ in range(C)]
    flat = {k: rep(v) for k, v in per_rec.items()}
    assert flat["language"] == [LANG_EN, LANG_EN, LANG_ZH, LANG_EN, LANG_EN]
    a, got, b, want = _split_and_flat(dict(STD, **per_rec), dict(STD, **flat))
    _assert_split_is_flat(a, got, b, want)
    assert [ch["language"] for rec in got for ch in rec["channels"]] == flat["language"]
    assert any(c[0] == "set_bias_rows" for c in a.calls)
    # values for all recordings stay as they are
    a, got, b, want = _split_and_flat(dict(STD, language=LANG_ZH, initial_prompt_tokens=[3, 4, 5], clip_timestamps="1,5,10,12"),
                                      dict(STD, language=LANG_ZH, initial_prompt_tokens=[3, 4, 5], clip_timestamps="1,5,10,12"))
    _assert_split_is_flat(a, got, b, want)
    # one entry per RECORDING is the rule: one per channel is refused, before any call
    for name in per_rec:
        ctx = ChanCtx(SPLIT_SCRIPT)
        with pytest.raises(ValueError):
            _run(ctx, _multi(), sample_rates=RATES, channels="split", **dict(STD, **{name: flat[name]}))
        assert ctx.calls == []


def test_split_recording_ids_are_per_channel_recording(tmp_path):
    ids = [7, 300, 65535, 0, 9]
    script = {(7, 1): HOT, (300, 0): SKIP, (65535, 1): HOT}
    a, got, b, want = _split_and_flat(dict(STD, recording_ids=ids), dict(STD, recording_ids=ids), script=script)
    _assert_split_is_flat(a, got, b, want)
    first = next(c for c in a.calls if c[0] == "transcribe_mel")
    assert [s & 0xFFFF for s in dict(first[2])["sample_ids"]] == ids
    for bad in ([0, 1, 2], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 65536]):          # one per recording is too few
        ctx = ChanCtx(SPLIT_SCRIPT)
        with pytest.raises(ValueError):
            _run(ctx, _multi(), sample_rates=RATES, channels="split", **dict(STD, recording_ids=bad))
        assert ctx.calls == []
    # the default: 0 .. 4
    a = ChanCtx(SPLIT_SCRIPT)
    _run(a, _multi(), sample_rates=RATES, channels="split", **STD)
    first = next(c for c in a.calls if c[0] == "transcribe_mel")
    assert [s & 0xFFFF for s in dict(first[2])["sample_ids"]] == [0, 1, 2, 3, 4]


def test_split_with_words_vad_and_reuse(tmp_path):
    """`It only changes what the recordings are`: a run with word timestamps, vad clips and a reused encoder"""
    vocab = make_vocab(tmp_path)
    try:
        t = _tracks()
        tracks = [t[0], t[0], t[1], t[2], t[2]]
        kw = dict(STD, vocab=vocab, word_timestamps=True, no_timestamps=NO_TS, vad=True, reuse_encoder=True, parallel_clips=2)
        a, got, b, want = _split_and_flat(kw, kw, tracks=tracks)
        _assert_split_is_flat(a, got, b, want)
        assert any("words" in sg for rec in got for sg in rec["segments"])
    finally:
        vocab.close()


def _activity():
    """recording 0 (7000 frames, 2 channels): left up to 35 s, right from there; recording 1 mono; recording 2 (1 frame): a tie"""
    left, right = np.zeros(7000, np.float32), np.zeros(7000, np.float32)
    left[:3500] = 3.0
    right[:3500] = 0.5
    right[3500:] = 2.0
    return [left, right, np.ones(3750, np.float32), np.ones(1, np.float32), np.ones(1, np.float32)]


def _strip(out):
    out = copy.deepcopy(out)
    for rec in out:
        for sg in rec["segments"]:
            del sg["speaker"]
            for w in sg.get("words", ()):
                del w["speaker"]
    return out


def test_diarize_is_the_plain_run_plus_one_mix_and_one_activity_call(tmp_path):
    vocab = make_vocab(tmp_path)
    try:
        for kw in (STD, dict(STD, vocab=vocab, word_timestamps=True, no_timestamps=NO_TS, language=LANGS)):
            a, b = ChanCtx(SCRIPT, activity=_activity()), ChanCtx(SCRIPT)
            got = _run(a, _multi(), sample_rates=RATES, channels="diarize", **kw)
            want = _run(b, _multi(), sample_rates=RATES, **kw)
            n = len(b.calls)
            assert a.calls[:n] == b.calls
            assert [c[0] for c in a.calls[n:]] == ["resample_16k_mix", "channel_activity", "dev_free"]
            mix_call, act_call, free_call = a.calls[n:]
            assert mix_call[1][1] == RATES and mix_call[1][2] == [np.eye(C).tolist() for C in COUNTS] and mix_call[2] == [["device", True]]
            assert act_call[1][0] == "ptr:8192" and act_call[1][1] == [0, 1120000, 2240000, 2840000, 2840160, 2840320]
            assert free_call[1] == ["ptr:8192"]
            assert _j(_strip(got)) == _j(want)
            act = _activity()
            n_seg = 0
            for rec, lo, C in zip(got, (0, 2, 3), COUNTS):
                for sg in rec["segments"]:
                    n_seg += 1
                    assert "speaker" in sg and sg["speaker"] == B.speaker_by_channel(act[lo:lo + C], sg["start"], sg["end"], 1.1)
                    for w in sg.get("words", ()):
                        assert w["speaker"] == B.speaker_by_channel(act[lo:lo + C], w["start"], w["end"], 1.1)
            assert n_seg >= 4
            speakers = [sg["speaker"] for sg in got[0]["segments"]]
            assert 0 in speakers and 1 in speakers                                            # both halves of recording 0 were heard
            assert all(sg["speaker"] is None for sg in got[1]["segments"]) and got[1]["segments"]   # mono
            if "vocab" in kw:
                assert any(w["speaker"] == 0 for sg in got[0]["segments"] for w in sg["words"])
    finally:
        vocab.close()


def test_diarize_channel_ratio_reaches_the_rule():
    a = ChanCtx(SCRIPT, activity=_activity())
    got = _run(a, _multi(), sample_rates=RATES, channels="diarize", channel_ratio=7.0, **STD)     # 3.0 : 0.5 is 6
    assert got[0]["segments"] and all(sg["speaker"] in (None, 1) for sg in got[0]["segments"])
    assert any(sg["speaker"] == 1 for sg in got[0]["segments"])


def test_channels_none_makes_the_calls_of_before():
    a, b = ChanCtx(SCRIPT), ChanCtx(SCRIPT)
    got = _run(a, _multi(), sample_rates=RATES, channels=None, channel_ratio=3.0, **STD)
    want = _run(b, _multi(), sample_rates=RATES, **STD)
    assert a.calls == b.calls and _j(got) == _j(want)
    assert not any(c[0] in ("resample_16k_mix", "channel_activity") for c in a.calls)
    assert all("speaker" not in sg and "channel" not in sg for rec in got for sg in rec["segments"])


@pytest.mark.parametrize("kw", [
    dict(channels="both", sample_rates=RATES),
    dict(channels="Split", sample_rates=RATES),
    dict(channels=True, sample_rates=RATES),
    dict(channels=2, sample_rates=RATES),
    dict(channels="split"),
    dict(channels="diarize"),
    dict(channels="split", sample_rates=RATES[:2]),
    dict(channels="diarize", sample_rates=RATES, channel_ratio=0.9),
    dict(channels="split", sample_rates=RATES, channel_ratio=float("nan")),
    dict(channels="diarize", sample_rates=RATES, channel_ratio=float("inf")),
    dict(channels="diarize", sample_rates=RATES, channel_ratio=None),
    dict(channels=None, sample_rates=RATES, channel_ratio=0.0),
])
def test_every_value_error_comes_before_any_call(kw):
    ctx = ChanCtx(SCRIPT, activity=_activity())
    with pytest.raises(ValueError):
        _run(ctx, _multi(), **dict(STD, **kw))
    assert ctx.calls == []


def test_a_recording_that_is_no_frame_array_is_refused_before_any_call():
    ctx = ChanCtx(SCRIPT)
    with pytest.raises(ValueError):
        _run(ctx, [np.zeros((10, 2, 2), np.float32)], sample_rates=[16000], channels="split", **STD)
    with pytest.raises(ValueError):
        _run(ctx, [np.zeros((10, 9), np.float32)], sample_rates=[16000], channels="diarize", **STD)
    assert ctx.calls == []


def test_no_recordings():
    for mode in ("split", "diarize"):
        ctx = ChanCtx(SCRIPT)
        assert _run(ctx, [], sample_rates=[], channels=mode, **STD) == []
        assert [c[0] for c in ctx.calls] == ["set_timestamp_rules"]
