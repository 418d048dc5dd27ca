"""GPU tests of transcribe_long's clip_timestamps, hallucination_silence_threshold and carry_initial_prompt through the
real library, on the lively tiny model with the production vocabulary (tests/test_longform_gpu.py: prod).  Every comparison
is exact: against the run without the argument, against the library's own single-row call, batched against alone.  The
rules themselves are pinned on the CPU (tests/test_longform_clips_cpu.py)."""
import pytest

from test_longform_gpu import EOT2, NS, SOT, SOT_PREV, TASK, _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import NO_TS2, prod_vocab  # noqa: F401  (prod_vocab: fixture)

pytestmark = pytest.mark.gpu

IDS = [7, 300, 65535]
SECONDS = [62.0, 45.0, 38.25]
# a clip shorter than one window that starts off a multiple of 3000, an odd count (the last clip runs to the end); no clip at
# all; two short clips, the second across the 30 s mark
CLIPS = [[5.0, 12.5, 40.0], [], [3.21, 9.0, 28.07, 33.5]]
ONCE = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
# test_a_threshold_rule_fires: the run's windows and tags as counted on an MI355X
FIRES = dict(threshold=2.0, seed=0, windows=26, leading=11, surrounded=15)


def _recs():
    tone = _long_recs()[2]
    return [tone[:int(16000 * SECONDS[0])], tone[5000:5000 + int(16000 * SECONDS[1])], tone[:int(16000 * SECONDS[2])]]


def _content(x):
    return (x.size + 480000) // 160 - 3000


def _pairs(times, content):
    """the (start, end) frames of the clips as given, cut at the recording's end"""
    p = [round(t * 100) for t in times] or [0]
    if len(p) % 2:
        p.append(content)
    return [(min(a, content), min(b, content)) for a, b in zip(p[::2], p[1::2])]


def _words_kw(vocab, **extra):
    return _kw(vocab=vocab, word_timestamps=True, no_timestamps=NO_TS2, **extra)


def _alone(prod, recs, clips, kw):
    return [prod.transcribe_long([x], recording_ids=[IDS[r]], clip_timestamps=None if clips is None else [clips[r]], **kw)[0]
            for r, x in enumerate(recs)]


def _check_seeks_grow_within_a_clip(out):
    for o in out:
        last = {}
        for w in o["windows"]:
            c = w.get("clip", 0)
            assert c not in last or w["seek"] > last[c], (c, o["seeks"])
            assert not last or c >= max(last), o["windows"]
            last[c] = w["seek"]


# ---------------------------------------------------------------- 1.
def test_a_clip_of_the_whole_recording_is_the_default_run(prod):
    recs = _recs()
    want = prod.transcribe_long(recs, recording_ids=IDS, **_kw())
    got = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=[[0, s] for s in SECONDS], **_kw())
    assert sum(len(o["windows"]) for o in want) >= 5
    for g, w in zip(got, want):
        assert all(x.pop("clip") == 0 for x in g["windows"])
        assert g == w
    flat = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps="0", **_kw())
    for g, w in zip(flat, want):
        assert [dict(x, clip=None) for x in g["windows"]] == [dict(x, clip=None) for x in w["windows"]]
        assert g["segments"] == w["segments"]


# ---------------------------------------------------------------- 2.
def test_the_windows_are_the_clips_and_decode_as_single_rows(prod):
    recs = _recs()
    times = [5.0, 12.5, 40.0]
    out = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=times, **_kw(**ONCE))
    n_ctx = prod.dims["n_text_ctx"]
    short = 0
    for r, (o, x) in enumerate(zip(out, recs)):
        content = _content(x)
        pairs = _pairs(times, content)
        mel = prod.logmel_long([x])[0]
        assert [w["clip"] for w in o["windows"]] == sorted(w["clip"] for w in o["windows"]) and o["windows"][0]["seek"] == 500
        assert {w["clip"] for w in o["windows"]} == {k for k, (a, b) in enumerate(pairs) if a < b}
        for k, w in enumerate(o["windows"]):
            a, b = pairs[w["clip"]]
            assert a <= w["seek"] < b, (r, w["seek"])
            assert w["segment_size"] == min(3000, content - w["seek"], b - w["seek"])
            assert w["temperatures"] == [0.0] and w["prompt"] == [SOT, o["language"], TASK]
            short += w["segment_size"] < 3000
            one = prod.transcribe_mel(mel, [0], mel.shape[1], w["seek"], w["segment_size"], [w["prompt"]], n_ctx // 2,
                                      eot=EOT2, no_speech_token=NS, sample_ids=[(k << 16) | IDS[r]])
            assert w["tokens"] == [int(t) for t in one.tokens[0, :one.n_text[0]]], (r, w["seek"])
        assert all(any(a <= s["seek"] < b for a, b in pairs) for s in o["segments"])
    assert short >= 3
    _check_seeks_grow_within_a_clip(out)


# ---------------------------------------------------------------- 3.
@pytest.mark.parametrize("words", [False, True])
def test_batched_clips_equal_each_recording_alone(prod, prod_vocab, words):
    recs = _recs()
    kw = _words_kw(prod_vocab, **ONCE) if words else _kw(**ONCE)
    got = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, **kw)
    assert got == _alone(prod, recs, CLIPS, kw)
    # the recording without a clip list is the recording of a run without the argument
    plain = prod.transcribe_long(recs[1:2], recording_ids=IDS[1:2], **kw)[0]
    assert [{k: v for k, v in w.items() if k != "clip"} for w in got[1]["windows"]] == plain["windows"]
    assert got[1]["segments"] == plain["segments"]
    assert got[0]["seeks"][0] == 500 and got[2]["seeks"][0] == 321 and got[2]["windows"][0]["segment_size"] <= 579
    assert {w["clip"] for w in got[2]["windows"]} == {0, 1}
    _check_seeks_grow_within_a_clip(got)


# ---------------------------------------------------------------- 4.
def test_encoder_reuse_with_clips_and_the_threshold(prod, prod_vocab):
    recs = _recs()
    kw = _words_kw(prod_vocab, hallucination_silence_threshold=FIRES["threshold"], seed=FIRES["seed"])
    a = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, **kw)
    b = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, reuse_encoder=True, **kw)
    assert a == b and sum(len(o["windows"]) for o in a) >= 5


# ---------------------------------------------------------------- 5.
def test_the_threshold_batched_equals_alone_and_the_seeks_grow(prod, prod_vocab):
    recs = _recs()
    kw = _words_kw(prod_vocab, hallucination_silence_threshold=FIRES["threshold"], seed=FIRES["seed"])
    got = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, **kw)
    assert got == _alone(prod, recs, CLIPS, kw)
    _check_seeks_grow_within_a_clip(got)
    for o in got:
        assert [s["id"] for s in o["segments"]] == list(range(len(o["segments"])))
        tagged = {w["seek"] for w in o["windows"] if w.get("hallucination") == "leading"}
        assert not any(s["seek"] in tagged for s in o["segments"])


# ---------------------------------------------------------------- 6.
def test_a_threshold_rule_fires(prod, prod_vocab):
    """hallucination_silence_threshold 2.0, seed 0, the default fallback temperatures, no clips.  A random-init model
    gives low word probabilities and many zero-length words, so anomalous segments are common: on an MI355X the run has 26 windows, 11 tagged
    "leading" and 15 "surrounded" (sampling is seeded, so the counts are exact)."""
    recs = _recs()
    kw = _words_kw(prod_vocab, hallucination_silence_threshold=FIRES["threshold"], seed=FIRES["seed"])
    got = prod.transcribe_long(recs, recording_ids=IDS, **kw)
    tags = [w.get("hallucination") for o in got for w in o["windows"]]
    print("hallucination tags: %d windows, %d leading, %d surrounded" % (len(tags), tags.count("leading"),
                                                                        tags.count("surrounded")))
    assert tags.count("leading") + tags.count("surrounded") >= 1
    assert (len(tags), tags.count("leading"), tags.count("surrounded")) == (FIRES["windows"], FIRES["leading"], FIRES["surrounded"])
    for o in got:
        for w in o["windows"]:
            assert ("dropped_segments" in w) == (w.get("hallucination") == "surrounded")
            assert w.get("dropped_segments", 1) >= 1
    _check_seeks_grow_within_a_clip(got)


# ---------------------------------------------------------------- 7.
def test_the_carried_prompt(prod):
    recs = _recs()
    ips = [[400, 401, 402], [], [500 + k for k in range(12)]]
    # (one decode per window at temperature 0: the synthetic model fails the log-prob test at every temperature, and a window
    # that ends at temperature 1.0 restarts the history behind itself -- that case is pinned on the CPU)
    kw = _kw(condition_on_previous_text=True, sot_prev=SOT_PREV, initial_prompt_tokens=ips, carry_initial_prompt=True, **ONCE)
    got = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, **kw)
    cap = prod.dims["n_text_ctx"] // 2 - 1
    longer = 0
    for r, o in enumerate(got):
        assert len(o["windows"]) >= 2
        hist = []      # the tokens of the segments of the windows so far (temperature 0: the history never restarts)
        for w in o["windows"]:
            if ips[r]:
                assert w["prompt"][:1 + len(ips[r])] == [SOT_PREV] + ips[r]
                text = ips[r] + hist[-(cap - len(ips[r])):]
            else:
                text = hist[-cap:]
            assert w["prompt"] == ([SOT_PREV] + text if text else []) + [SOT, o["language"], TASK], (r, w["seek"])
            assert len(w["prompt"]) == w["prompt_len"] <= 1 + cap + 3
            longer += len(w["prompt"]) > 1 + len(ips[r]) + 3
            hist += [t for s in o["segments"] if s["seek"] == w["seek"] for t in s["tokens"]]
    assert longer >= 2      # the history follows the carried prompt
    for r, x in enumerate(recs):
        alone = prod.transcribe_long([x], recording_ids=[IDS[r]], clip_timestamps=[CLIPS[r]],
                                     **dict(kw, initial_prompt_tokens=[ips[r]]))[0]
        assert alone == got[r], r
    off = prod.transcribe_long(recs, recording_ids=IDS, clip_timestamps=CLIPS, **dict(kw, carry_initial_prompt=False))
    assert off[1] == got[1]      # no initial prompt: nothing to carry
