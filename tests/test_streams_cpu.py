"""CPU tests of live streams: the f64 restatement of a stream's frames (tests/stream_ref.py) against the whole-recording
restatement, the frame counters against brute force, and the agreement policy of openai-whisper-coreml_amd/live.py as pure
functions on scripted hypothesis sequences (no GPU, no library)."""
import importlib
import os

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

import stream_ref as SR
from conftest import GOLDEN
from test_longform_cpu import long_log_mel_np

B = importlib.import_module("openai_whisper_coreml_amd.binding")
LV = importlib.import_module("openai_whisper_coreml_amd.live")

TB, EOT = 100, 50   # timestamp_begin and eot of the hand-built hypotheses; text ids are below 50


def _sig(n, seed=0):
    rng = np.random.default_rng(seed)
    return 0.2 * np.sin(np.arange(n) * 0.05) + 0.02 * rng.standard_normal(n)


@pytest.mark.parametrize("n", [1, 41, 200, 201, 360, 5000, 50001])
def test_stream_ref_first_window_is_the_long_form(n):
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    x = _sig(n)
    raw = SR.raw_frames(x, m80)
    A = SR.counts(n, 1 << 40)[1]
    assert raw.shape == (80, A)
    want = long_log_mel_np(x, m80)
    # frames >= A of the long form read no sample: all -10 before the clamp, never its maximum
    assert np.all(want[:, A:] == want[:, A:].min())
    assert np.abs(SR.window(raw, 0, A) - want[:, :A]).max() <= 1e-12


def test_stream_ref_later_window_and_placed_stream():
    m80 = np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201)
    x = _sig(8000, seed=1)
    raw = SR.raw_frames(x, m80)
    w = SR.window(raw, 7, 20)
    assert w.shape == (80, 20) and w.max() == (raw[:, 7:27].max() + 4.0) / 4.0 and w.min() >= w.max() - 2.0
    # a stream placed after 10 hops of silence: its frame j is frame 10 + j of the stream that got the silence as samples
    placed = SR.raw_frames(x, m80, from_start=False)
    whole = SR.raw_frames(np.concatenate([np.zeros(1600), x]), m80)
    assert np.abs(placed - whole[:, 10:10 + placed.shape[1]]).max() <= 1e-12


def test_frame_counters_against_brute_force():
    for n in range(0, 2001):
        want = SR.counts_brute(n, 5)
        assert SR.counts(n, 5) == want, n
        assert B.stream_frame_counts(n, 5) == want, n
        F, A, _ = want
        assert 0 <= A - F <= 3
    assert B.stream_frame_counts((1 << 33) + 1600, 3003) == (((1 << 33) + 1400) // 160 + 1, ((1 << 33) + 1799) // 160 + 1,
                                                              ((1 << 33) + 1799) // 160 + 1 - 3003)


# ---------------------------------------------------------------- the policy
def test_agreement_commits_the_common_prefix_of_two_hypotheses():
    s = LV.new_state()
    s, new = LV.agree(s, (TB, 1, 2, 3), TB)
    assert s.committed == () and s.prev == (TB, 1, 2, 3) and new.tokens == []
    s, new = LV.agree(s, (TB, 1, 2, 4, 5), TB)
    assert s.committed == (TB, 1, 2) and s.prev == (4, 5) and new.tokens == [TB, 1, 2]
    assert new.starts == [0.0, 0.0, 0.0]
    s, new = LV.agree(s, (TB, 1, 2, 4, 5, TB + 50, TB + 50, 6), TB)
    assert s.committed == (TB, 1, 2, 4, 5) and s.prev == (TB + 50, TB + 50, 6) and new.tokens == [4, 5]
    s, new = LV.agree(s, (TB, 1, 2, 4, 5, TB + 50, TB + 50, 6, 7), TB)
    assert new.tokens == [TB + 50, TB + 50, 6] and new.starts == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        LV.agree(s, (TB, 9), TB)   # a hypothesis that drops what it was given


def test_eot_is_never_committed():
    assert LV.hypothesis_of([TB, 1, 2, EOT, 7, 7], 6, EOT) == (TB, 1, 2)
    assert LV.hypothesis_of([TB, 1, 2, 3], 3, EOT) == (TB, 1, 2)
    assert LV.hypothesis_of([EOT], 1, EOT) == ()
    s = LV.new_state()
    for toks in ([TB, 1, EOT], [TB, 1, EOT], [TB, 1, 2, EOT]):
        s, new = LV.agree(s, LV.hypothesis_of(toks, len(toks), EOT), TB)
        assert EOT not in s.committed and EOT not in new.tokens and EOT not in s.prev


def test_trim_shifts_timestamps_and_keeps_buf_first_even():
    s = LV.StreamState(40, (TB, 1, 2, TB + 101, TB + 101, 3, TB + 150, TB + 150, 4), (5, TB + 330), (9,), 0)
    same, cut = LV.trim(s, 40 + 1500, 1500, TB)
    assert not cut and same == s                     # not more than trim_frames in the buffer
    t, cut = LV.trim(s, 40 + 1501, 1500, TB)
    assert cut
    assert t.buf_first == 40 + 2 * 150 and t.buf_first % 2 == 0
    assert t.committed == (TB, 4) and t.prev == (5, TB + 180)
    assert t.context == (9, 1, 2, 3)
    # no adjacent pair: nothing to cut at
    u = s._replace(committed=(TB, 1, 2, TB + 101))
    assert LV.trim(u, 5000, 1500, TB) == (u, False)
    # a pair whose time lies behind the audio that has arrived is no cut
    v = s._replace(buf_first=0, committed=(TB, 1, TB + 900, TB + 900))
    assert LV.trim(v, 1700, 1500, TB) == (v, False)
    # the absolute times of what stays are unchanged
    assert LV.token_starts(t.committed, 0, t.buf_first, TB) == LV.token_starts(s.committed, 7, s.buf_first, TB)


def test_forced_advance_with_and_without_tokens():
    # tokens, no pair: prev is committed whole, the buffer is cut at the last timestamp token
    s = LV.StreamState(0, (TB, 1, 2), (3, TB + 1400, 4), (), 0)
    t, new = LV.force_advance(s, 2950, 1500, TB)
    assert new.tokens == [3, TB + 1400, 4] and new.starts == [0.0, 28.0, 28.0]
    assert t.buf_first == 2800 and t.committed == (4,) and t.prev == () and t.context == (1, 2, 3)
    # no tokens at all: the even frame at or below avail - trim_frames
    t, new = LV.force_advance(LV.new_state(), 2951, 1500, TB)
    assert new.tokens == [] and t.buf_first == 1450 and t.committed == () and t.prev == ()
    # only <|0.00|>: the cut would not move the buffer
    t, new = LV.force_advance(LV.StreamState(10, (TB, 1), (2,), (), 0), 2960, 1500, TB)
    assert new.tokens == [2] and t.buf_first == 1460 and t.context == (1, 2) and t.committed == ()
    # after_hypothesis fires it exactly when the next step would exceed a window and no trim happened
    s = LV.StreamState(0, (), (TB, 1), (), 0)
    t, _ = LV.after_hypothesis(s, (TB, 1), 2900, 2898, timestamp_begin=TB)
    assert t.buf_first == 0 and t.committed == (TB, 1)
    t, _ = LV.after_hypothesis(s, (TB, 1), 2901, 2899, timestamp_begin=TB)
    assert t.buf_first == 1400 and t.context == (1,)
    # audio that outran the steps is advanced before the decode
    t, _ = LV.before_decode(LV.new_state(), 4001, 1500, TB)
    assert t.buf_first == 2500 and 4001 - t.buf_first <= 3000


def test_prompt_and_its_truncated_context():
    seq = [200, 201, 202]
    assert LV.stream_prompt((), seq, 199, 448) == seq
    assert LV.stream_prompt((1, 2), seq, 199, 448) == [199, 1, 2] + seq
    ctx = tuple(range(1, 40))
    p = LV.stream_prompt(ctx, seq, 199, 32)
    assert p == [199] + list(ctx[-15:]) + seq and len(p) == 1 + 15 + 3


def _text(tokens):
    return [t for t in tokens if t < TB]


@settings(max_examples=200, deadline=None)
@given(st.lists(st.lists(st.integers(0, 8), max_size=12), min_size=1, max_size=30), st.integers(50, 400),
       st.sampled_from([200, 600, 1500]))
def test_committed_text_is_prefix_monotone_over_any_script(script, avail_step, trim_frames):
    """Whatever the hypotheses say -- here: arbitrary continuations of the committed tokens, text ids and non-decreasing
    timestamps mixed -- the text a stream has committed only ever grows at its end, the tokens handed out are exactly that
    growth, buf_first stays even and inside the audio, and the buffer never exceeds a window."""
    s = LV.new_state()
    avail, said = 0, []
    for draws in script:
        avail += avail_step
        s, early = LV.before_decode(s, avail, trim_frames, TB)
        last_ts = max([t for t in s.committed if t >= TB], default=TB)
        tail = []
        for d in draws:   # 0 .. 5: a text id; 6 .. 8: a timestamp that does not go back, and stays inside the buffer
            if d >= 6:
                last_ts = min(last_ts + (d - 6) * 40, TB + max(0, (avail - s.buf_first - 1) // 2))
                tail.append(last_ts)
            else:
                tail.append(d)
        before = _text(s.context) + _text(s.committed)
        s, new = LV.after_hypothesis(s, tuple(s.committed) + tuple(tail), avail, avail - 2, timestamp_begin=TB,
                                     trim_frames=trim_frames, min_step_frames=avail_step)
        said += _text(early.tokens) + _text(new.tokens)
        after = _text(s.context) + _text(s.committed)
        assert after[:len(before)] == before
        assert after == said
        assert len(new.tokens) == len(new.starts) and all(b >= a for a, b in zip(new.starts, new.starts[1:]))
        assert s.buf_first % 2 == 0 and 0 <= s.buf_first < avail
        assert avail - s.buf_first <= 3000


def test_unserved_modes_raise():
    class Ctx:
        dims = {"n_text_ctx": 448, "n_mels": 80}
    ids = dict(sot=1, language=2, task=3, eot=EOT, timestamp_begin=TB, sot_prev=4)
    for kw in (dict(sample_rate=8000), dict(best_of=5), dict(beam_size=5), dict(temperatures=(0.0, 0.2))):
        with pytest.raises(ValueError):
            LV.LiveTranscriber(Ctx(), 2, **ids, **kw)
