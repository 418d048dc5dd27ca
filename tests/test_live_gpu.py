"""GPU tests of live.LiveTranscriber on the `lively` synthetic model of test_model_gpu.py: every step's hypothesis is token
for token what a plain transcribe_mel call gives on the audio so far under the same prompt and given tokens; streams
stepped together equal each alone; committed text only grows; a trim moves the buffer and the next step decodes the shifted
window with the shifted tokens given; finish commits the last hypothesis."""
import importlib

import numpy as np
import pytest

from test_model_gpu import lively, tones  # noqa: F401  (lively: fixture)
from test_transcribe_options_gpu import EOT, PROMPT, SPECIALS, TS

pytestmark = pytest.mark.gpu

LV = importlib.import_module("openai_whisper_coreml_amd.live")
IDS = dict(sot=PROMPT[0], language=PROMPT[1], task=PROMPT[2], eot=EOT, timestamp_begin=TS, sot_prev=SPECIALS[-2])
PACKET = 8000   # 0.5 s


@pytest.fixture(scope="module")
def audio():
    return [np.ascontiguousarray(tones(1, i)[0][:96000]) for i in range(3)]   # 6 s each


def _plain(ctx, b, mel, prompt, given, max_new):
    """one plain call on a host block [80][n]"""
    n = mel.shape[1]
    r = ctx.transcribe_mel(np.ascontiguousarray(mel), np.zeros(1, np.int64), n, 0, n, [prompt], max_new, eot=EOT, sot_tail=3,
                           given=[given] if given else None)
    return LV.hypothesis_of(r.tokens[0], r.lens[0], EOT)


def _run(ctx, streams_audio, packets, **kw):
    """push packets[s] samples per round to stream s and step after every round; per stream the list of (samples so far,
    first, n, prompt, given, hypothesis, Committed, tail) of its steps, and the transcriber's final commits"""
    S = len(streams_audio)
    log = [[] for _ in range(S)]
    with LV.LiveTranscriber(ctx, S, **IDS, **kw) as lt:
        at = [0] * S
        while any(at[s] < len(streams_audio[s]) for s in range(S)):
            pieces = []
            for s in range(S):
                pieces.append(streams_audio[s][at[s]:at[s] + packets[s]] if at[s] < len(streams_audio[s]) else None)
                at[s] = min(at[s] + packets[s], len(streams_audio[s]))
            lt.push(pieces)
            for s, (new, tail) in lt.step().items():
                log[s].append((at[s],) + lt.last[s] + (new, tail))
        last_prev = [lt.state[s] for s in range(S)]
        fin = [lt.finish(s) for s in range(S)]
        assert all(int(v) == 0 for v in lt.streams.frames()[0])
    return log, last_prev, fin


def test_every_step_is_a_plain_call_on_the_audio_so_far(lively, pkg, audio):
    _, _, _, ctx = lively
    b = pkg.binding
    ctx.set_suppress(SPECIALS, [EOT])
    try:
        log, state, fin = _run(ctx, audio[:1], [PACKET])
        assert len(log[0]) >= 5
        said = []
        for n_samples, first, n, prompt, given, hyp, new, tail in log[0]:
            assert first == 0 and n == b.stream_frame_counts(n_samples, 3003)[1]
            mel = ctx.logmel_long([audio[0][:n_samples]])[0][:, :n]
            assert hyp == _plain(ctx, b, mel, prompt, given, 221)
            assert list(given) == said and EOT not in hyp       # what was committed is given, and only grows
            said += new.tokens
            assert list(hyp[:len(said)]) == said and list(hyp[len(said):]) == tail
        # finish decodes the whole audio once more and commits that hypothesis whole
        mel = ctx.logmel_long([audio[0]])[0][:, :b.stream_frame_counts(96000, 3003)[1]]
        prompt = LV.stream_prompt(state[0].context, [IDS["sot"], IDS["language"], IDS["task"]], IDS["sot_prev"], 448)
        last = _plain(ctx, b, mel, prompt, list(state[0].committed), 221)
        assert said + fin[0].tokens == list(last) and len(fin[0].starts) == len(fin[0].tokens)
    finally:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])


def test_streams_together_equal_each_alone(lively, pkg, audio):
    _, _, _, ctx = lively
    ctx.set_suppress(SPECIALS, [EOT])
    try:
        packets = [PACKET, 5000, 12000]
        together, _, fin = _run(ctx, audio, packets, min_step_frames=60)
        assert len({len(l) for l in together}) > 1        # the streams were due at different rounds
        for s in range(3):
            alone, _, fin1 = _run(ctx, [audio[s]], [packets[s]], min_step_frames=60)
            assert [e[:6] for e in alone[0]] == [e[:6] for e in together[s]]
            assert [(e[6].tokens, e[6].starts, e[7]) for e in alone[0]] == [(e[6].tokens, e[6].starts, e[7]) for e in together[s]]
            assert fin1[0] == fin[s]
            text = []
            for e in together[s]:                         # committed text is prefix-monotone
                assert list(e[4]) == text
                text += e[6].tokens
    finally:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])


def test_a_trim_and_the_step_after_it(lively, pkg, audio):
    """trim_frames = 200.  The committed tokens of the second step are planted with an adjacent timestamp pair (a given row
    decodes them as they are), so the trim does not hang on what the synthetic model says."""
    _, _, _, ctx = lively
    b = pkg.binding
    ctx.set_suppress(SPECIALS, [EOT])
    x = audio[1]
    try:
        with LV.LiveTranscriber(ctx, 1, **IDS, trim_frames=200, min_step_frames=50) as lt, b.Streams(ctx, 1) as whole:
            lt.push([x[:40000]])
            assert 0 in lt.step()
            planted = (TS, 30, 31, TS + 60, TS + 60, 32)
            lt.state[0] = lt.state[0]._replace(committed=planted, prev=())
            lt.push([x[40000:56000]])
            out = lt.step()
            first, n, prompt, given, hyp = lt.last[0]
            assert first == 0 and tuple(given) == planted and hyp[:6] == planted and prompt == PROMPT
            s = lt.state[0]
            assert s.buf_first == 120 and s.context == (30, 31) and s.committed[:2] == (TS, 32)      # the trim happened
            assert all(t - 60 == u for t, u in zip([v for v in hyp[6:] if v >= TS],
                                                   [v for v in s.committed[2:] + s.prev if v >= TS]))
            assert out[0][0].tokens == list(s.committed[2:])
            lt.push([x[56000:72000]])
            lt.step()
            first, n, prompt, given, hyp = lt.last[0]
            A = b.stream_frame_counts(72000, 3003)[1]
            assert (first, n) == (120, A - 120) and prompt == [IDS["sot_prev"], 30, 31] + PROMPT and tuple(given) == s.committed
            # the plain call on the shifted window of a stream that got the audio in one push
            whole.push([x[:72000]])
            mel = whole.window([(0, 120, A - 120)], device=False)[0]
            assert hyp == _plain(ctx, b, mel, prompt, list(given), 221)
            assert lt.state[0].buf_first % 2 == 0
    finally:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])


def test_unserved_modes_raise(lively):
    _, _, _, ctx = lively
    for kw in (dict(sample_rate=44100), dict(best_of=3), dict(beam_size=4), dict(temperatures=(0.0, 0.4))):
        with pytest.raises(ValueError):
            LV.LiveTranscriber(ctx, 1, **IDS, **kw)
