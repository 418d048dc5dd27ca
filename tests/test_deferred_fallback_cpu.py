"""binding.transcribe_long(fallback="deferred") against the lockstep loop on a scripted fake context (the recording fake of
test_longform_calls_cpu, subclassed): a script says, per window and attempt, whether the attempt fails.

The fake checks every row of every decode call itself: attempt k of a window arrives at temperatures[k] with seed
fallback_seed(seed, k), under the window's sample id, only after attempt k - 1 failed.

Decode calls.  Without parallel_clips the counts are exact: with a(u, r) attempts of window r of recording u, the lockstep loop
makes sum_r max_u a(u, r) calls and the deferred loop max_u sum_r a(u, r) -- never more, and fewer exactly when no recording holds
the round's maximum in every round.  (A window that falls back beside one that does not is NOT enough for "strictly fewer": two
recordings of one window each with 2 and 1 attempts take 2 calls either way.)  The seeded scripts must show the strict case."""
import importlib

import numpy as np
import pytest

from test_longform_calls_cpu import MIN, STD, RecCtx, make_vocab
from test_longform_clips_cpu import DEFAULT, _rec
from test_longform_words_cpu import EOT, NO_TS

B = importlib.import_module("openai_whisper_coreml_amd.binding")
ROUND_ROWS = B._RoundRows
TEMPS = (0.0, 0.2, 0.4, 0.6)
SEED = 11


class ScriptCtx(RecCtx):
    """fails[(recording id, sample id >> 16)] = n: attempts 0 .. n - 1 of that window fail (n may exceed the temperatures: the
    last attempt is kept); skips: windows the silence rule skips.  rows: per decode call [(sample id, attempt)]."""

    def __init__(self, fails, skips, temperatures=TEMPS, seed=SEED):
        RecCtx.__init__(self, {})
        self.fails, self.skips, self.temps, self.seed = fails, skips, [float(t) for t in temperatures], seed
        self.attempts, self.rows, self.mixed = {}, [], 0

    def _decode(self, ids, max_new, kw):
        n, eot = len(ids), kw["eot"]
        ts = kw.get("row_temperatures", [kw["temperature"]] * n)
        sds = kw.get("row_seeds", [kw["seed"]] * n)
        assert len(ts) == len(sds) == n
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.full(n, 0.01, dtype=np.float32)
        call = []
        for i, sid in enumerate(ids):
            key = (int(sid) & 0xFFFF, int(sid) >> 16)
            k = self.attempts.get(key, 0)
            assert k < len(self.temps) and (k == 0 or k <= self.fails.get(key, 0)), (key, k)   # it comes back only after a failure
            assert float(ts[i]) == self.temps[k] and int(sds[i]) == B.fallback_seed(self.seed, k), (key, k, ts[i], sds[i])
            self.attempts[key] = k + 1
            call.append((int(sid), k))
            body = ([] if key in self.skips else list(DEFAULT["tokens"])) + [eot]
            toks[i, :len(body)] = body
            lens[i] = len(body)
            lp[i, :len(body)] = -5.0 if k < self.fails.get(key, 0) else -0.1 - 0.01 * k   # (the kept attempt shows in avg_logprob)
            if key in self.skips:
                ns[i], lp[i, :len(body)] = 0.9, -5.0
        self.rows.append(call)
        self.mixed += len({k for _, k in call}) > 1
        return B.TranscribeResult(toks, lens, lp, ns, eot)


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def script(rng, R):
    fails, skips = {}, set()
    for r in range(R):
        for n in range(64):
            x = rng.random()
            if x < 0.3:
                fails[(r, n)] = int(rng.integers(1, len(TEMPS) + 2))
            elif x < 0.4:
                skips.add((r, n))
    return fails, skips


def run(monkeypatch, fails, skips, recs, mode, **kw):
    rounds = []

    class Counting(ROUND_ROWS):
        def __init__(self, *a, **k):
            rounds.append(1)
            ROUND_ROWS.__init__(self, *a, **k)
    monkeypatch.setattr(B, "_RoundRows", Counting)
    ctx = ScriptCtx(fails, skips)
    out = B.transcribe_long(ctx, recs, temperatures=TEMPS, seed=SEED, fallback=mode, **kw)
    ctx.n_rounds = len(rounds)
    ctx.n_calls = sum(c[0] in ("transcribe_mel", "transcribe_mel_aligned") for c in ctx.calls)
    assert ctx.n_calls == len(ctx.rows)
    return ctx, out


def without_rounds(out):
    return [dict(o, windows=[{k: v for k, v in w.items() if k != "round"} for w in o["windows"]]) for o in out]


CASES = {
    "plain": dict(STD),
    "conditioned": dict(STD, condition_on_previous_text=True, prompt_reset_on_temperature=0.3),
    "words": dict(STD, word_timestamps=True, no_timestamps=NO_TS),
    "conditioned_words": dict(STD, condition_on_previous_text=True, word_timestamps=True, no_timestamps=NO_TS),
    "parallel_clips": dict(STD, clip_timestamps=[0.0, 22.0, 30.0, 41.0, 50.0, 58.0], parallel_clips=3),
    "parallel_words": dict(STD, clip_timestamps=[0.0, 45.0, 50.0, 68.0], parallel_clips=True, word_timestamps=True, no_timestamps=NO_TS),
}


def compare(monkeypatch, vocab, name, seed):
    """-> (decode calls saved, deferred calls that mixed attempts)"""
    rng = np.random.default_rng(100 * seed + len(name))
    kw = dict(CASES[name])
    if "word_timestamps" in kw:
        kw["vocab"] = vocab
    recs = [_rec(s) for s in (70.0, 37.5, 61.0, 0.01)]
    fails, skips = script(rng, len(recs))
    lock, want = run(monkeypatch, fails, skips, recs, "lockstep", **kw)
    defer, got = run(monkeypatch, fails, skips, recs, "deferred", **kw)
    assert without_rounds(got) == without_rounds(want)
    assert any(len(w["temperatures"]) > 1 for o in want for w in o["windows"])           # a window fell back ...
    assert any(len(w["temperatures"]) == 1 for o in want for w in o["windows"])          # ... and one did not
    assert defer.n_calls == defer.n_rounds                                               # one decode call per round
    assert all("row_temperatures" in dict(c[2]) for c in defer.calls if c[0].startswith("transcribe_mel"))
    assert defer.attempts == lock.attempts                                               # the same attempts of the same windows
    assert defer.n_calls <= lock.n_calls
    if "parallel_clips" not in kw:   # the exact counts (module docstring)
        a = [[len(w["temperatures"]) for w in o["windows"]] for o in want]
        depth = max(len(x) for x in a)
        assert lock.n_calls == sum(max(x[r] for x in a if len(x) > r) for r in range(depth))
        assert defer.n_calls == max(sum(x) for x in a)
    return lock.n_calls - defer.n_calls, defer.mixed


@pytest.mark.parametrize("name", list(CASES))
def test_deferred_equals_lockstep_with_one_call_per_round(monkeypatch, vocab, name):
    """over seeded random scripts: equal results, one call per round, the expected rows, never more calls -- and the scripts of
    every case do show fewer calls and calls that mix attempts"""
    saved = mixed = 0
    for seed in (1, 2, 3, 4):
        d, m = compare(monkeypatch, vocab, name, seed)
        saved += d > 0
        mixed += m > 0
    assert saved >= 1 and mixed >= 1, (saved, mixed)


def test_a_window_that_falls_back_beside_one_that_does_not(monkeypatch):
    """Two recordings of two windows; window 0 of recording 0 and window 1 of recording 1 need two attempts: 2 + 2 lockstep
    calls, max(3, 3) deferred ones, and the second deferred call holds attempt 1 of the first beside attempt 0 of
    window 1 of the other recording."""
    recs = [_rec(37.5), _rec(37.5)]
    fails = {(0, 0): 1, (1, 1): 1}
    lock, want = run(monkeypatch, fails, set(), recs, "lockstep", **STD)
    defer, got = run(monkeypatch, fails, set(), recs, "deferred", **STD)
    assert without_rounds(got) == without_rounds(want)
    assert [len(o["windows"]) for o in want] == [2, 2]
    assert (lock.n_calls, defer.n_calls) == (4, 3)
    assert sorted(defer.rows[1]) == [(0 | (0 << 16), 1), (1 | (1 << 16), 0)]
    assert want[0]["windows"][0]["temperatures"] == [0.0, 0.2] and got[0]["segments"][0]["temperature"] == 0.2
    assert got[1]["windows"][1]["temperatures"] == [0.0, 0.2]


def test_value_errors_come_before_any_library_call():
    for kw in (dict(fallback="eager"), dict(fallback=None), dict(fallback="deferred", best_of=3), dict(fallback="deferred", beam_size=2),
               dict(fallback="deferred", draft=object()), dict(fallback="deferred", reuse_encoder=True)):
        ctx = ScriptCtx({}, set())
        with pytest.raises(ValueError):
            B.transcribe_long(ctx, [_rec(31.0)], **dict(STD, **kw))
        assert ctx.calls == []
    for bad in (dict(row_temperatures=[0.0]), dict(row_seeds=[1])):
        with pytest.raises(ValueError):
            B.sampling_rows_args(bad.get("row_temperatures"), bad.get("row_seeds"))
    with pytest.raises(ValueError):
        B.sampling_rows_args([0.0, 0.2], [1])
    assert B.sampling_rows_args(None, None) is None


def test_the_decision_function_is_fallback_decodes():
    """needs_fallback on the cases of test_fallback_decode_is_the_rule_of_transcribe_with_fallback (row 1 bad until T = 0.4), and
    on every combination of the three thresholds"""
    def decode(todo, t, sd):
        n = len(todo)
        toks = np.full((n, 4), EOT, dtype=np.int32)
        toks[:, 0] = 7
        lp = np.array([[-2.0 if (b == 1 and t < 0.4) else -0.1, -0.1, 0, 0] for b in todo], dtype=np.float32)
        return B.TranscribeResult(toks, np.full(n, 2, dtype=np.int32), lp, np.zeros(n, np.float32), EOT)
    for temps in ((0.0,), (0.0, 0.2), (0.0, 0.2, 0.4)):
        out = B.fallback_decode(decode, 3, 1024, 4, EOT, temperatures=temps, seed=5, compression_ratio_threshold=None)
        for b in range(3):
            want = B.needs_fallback(out["compression_ratio"][b], out["avg_logprob"][b], out["no_speech_prob"][b], None, -1.0, 0.6)
            assert bool(out["needs_fallback"][b]) == want == (b == 1 and temps[-1] < 0.4)
    for cr in (1.0, 3.0):
        for lp in (-0.5, -2.0):
            for ns in (None, 0.1, 0.9):
                for crt in (None, 2.4):
                    for lpt in (None, -1.0):
                        for nst in (None, 0.6):
                            want = (crt is not None and cr > crt) or (lpt is not None and lp < lpt)
                            if nst is not None and ns is not None and ns > nst:
                                want = False
                            assert B.needs_fallback(cr, lp, ns, crt, lpt, nst) == want
