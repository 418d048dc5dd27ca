"""binding.transcribe_long(fallback="deferred") on the GPU: three short synthetic recordings on the lively tiny model with the
production vocabulary.  logprob_threshold is the median temperature-0 avg_logprob of a first lockstep run, so about half of the
windows fall back; the deferred run -- one decode call per round, every row at its own temperature and seed
(wm_set_sampling_rows) -- must equal the lockstep run per recording in language, segments, seeks and window records (their round
numbers aside), and the test asserts that it is not vacuous."""
import numpy as np
import pytest

from test_longform_gpu import _kw, _long_recs, prod  # noqa: F401  (prod: module fixture)
from test_longform_words_gpu import prod_vocab  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu

TEMPS = (0.0, 0.5, 1.0)


def recordings():
    tone = _long_recs()[2]
    # (two or three windows each: a window kept at temperature 0 has a successor that can ride beside another's fallback)
    return [tone[:65 * 16000 + 123], tone[5000:5000 + 45 * 16000], tone[20000:20000 + 50 * 16000]]


def without_rounds(out):
    return [dict(o, windows=[{k: v for k, v in w.items() if k != "round"} for w in o["windows"]]) for o in out]


@pytest.fixture(scope="module")
def threshold(prod):
    """the median avg_logprob of the windows a temperature-0 lockstep run keeps"""
    out = prod.transcribe_long(recordings(), recording_ids=[4, 9, 300], temperatures=(0.0,), compression_ratio_threshold=None,
                               logprob_threshold=None, **_kw())
    lps = [{sg["seek"]: sg["avg_logprob"] for sg in o["segments"]} for o in out]
    values = sorted(v for d in lps for v in d.values())
    assert len(values) >= 4 and values[0] < values[-1], values
    return float(np.median(values))


@pytest.mark.parametrize("words", [False, "decode"])
def test_deferred_equals_lockstep(prod, prod_vocab, threshold, monkeypatch, words):
    kw = _kw(recording_ids=[4, 9, 300], temperatures=TEMPS, seed=21, compression_ratio_threshold=None, logprob_threshold=threshold)
    if words:
        kw.update(word_timestamps=words, vocab=prod_vocab)
    calls = []
    for name in ("transcribe_mel", "transcribe_mel_aligned"):
        real = getattr(prod, name)

        def spy(*a, _real=real, **k):
            calls.append(k.get("row_temperatures"))
            return _real(*a, **k)
        monkeypatch.setattr(prod, name, spy)
    want = prod.transcribe_long(recordings(), **kw)
    n_lock = len(calls)
    assert all(c is None for c in calls)
    got = prod.transcribe_long(recordings(), fallback="deferred", **kw)
    rows = calls[n_lock:]
    assert without_rounds(got) == without_rounds(want)
    # not vacuous
    temps = [w["temperatures"] for o in want for w in o["windows"]]
    assert any(t == [0.0] for t in temps), temps            # a window was kept at temperature 0
    assert any(len(t) > 1 for t in temps), temps            # a window fell back
    assert all(r is not None for r in rows)
    assert any(len(set(r)) > 1 for r in rows), rows         # a call mixed rows of different temperatures
    assert len(rows) <= n_lock
    print("decode calls: lockstep %d, deferred %d; windows %d, fell back %d" % (n_lock, len(rows), len(temps),
                                                                               sum(len(t) > 1 for t in temps)))
