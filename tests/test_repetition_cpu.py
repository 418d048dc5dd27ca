"""The repetition rules without a device: the numpy restatement (tests/repeat_ref.py) against a brute-force enumeration, the
wrapper's packing against a stand-in library, and transcribe_long's calls on the recording fake of
test_longform_calls_cpu.py."""
import ctypes
import importlib

import numpy as np
import pytest

import repeat_ref as RR
from test_longform_calls_cpu import RecCtx, cases, make_vocab, run_case, canon
from test_longform_clips_cpu import _rec
from test_longform_calls_cpu import SECONDS

B = importlib.import_module("openai_whisper_coreml_amd.binding")


# ---------------------------------------------------------------- the restatement against a brute force
def brute_ban(g, n, eot, V):
    """By the meaning of the rule: t is banned iff appending it makes the LAST n-gram of g + [t] equal an earlier n-gram."""
    g = [int(t) for t in g]
    out = set()
    if n <= 0:
        return out
    for t in range(min(eot, V)):
        h = g + [t]
        if len(h) < n:
            continue
        last = h[len(h) - n:]
        for i in range(len(h) - n):            # earlier n-grams: they end before the appended token
            if h[i:i + n] == last:
                out.add(t)
                break
    return out


def histories(rng, k, V):
    yield "random", rng.integers(0, V, k)
    yield "few ids", rng.integers(0, 4, k)
    yield "all equal", np.full(k, 3)
    yield "period 2", np.tile([5, 9], k // 2 + 1)[:k]
    yield "period 3 with an id >= eot inside", np.tile([5, V - 1, 9], k // 3 + 1)[:k]


@pytest.mark.parametrize("n", [1, 2, 3, 8, 32])
def test_ban_set_against_the_brute_force(n):
    V, eot = 24, 20                                 # ids 20 .. 23 are never banned but stand in the history
    rng = np.random.default_rng(100 + n)
    for k in sorted({0, max(n - 2, 0), n - 1, n, n + 1, 2 * n + 1, 447}):
        for name, g in histories(rng, k, V):
            want = brute_ban(g, n, eot, V)
            assert RR.ban_set(g, n, eot) == want, (n, k, name)
            assert all(t < eot for t in want)
            if k < n:
                assert not want, (n, k, name)
            if n == 1:
                assert want == RR.seen_set(g, eot)


def test_hand_made_histories():
    eot = 10
    assert RR.ban_set([1, 2, 3, 1, 2], 3, eot) == {3}
    assert RR.ban_set([1, 2, 3, 1, 2], 2, eot) == {3}             # suffix [2]: followed by 3 once
    assert RR.ban_set([1, 2, 1, 2, 1], 2, eot) == {2}
    assert RR.ban_set([7, 7, 7], 3, eot) == {7}                   # all equal: starts at 0 only (i <= k - n)
    assert RR.ban_set([7, 7], 3, eot) == set()                    # k = n - 1: a suffix, but no start
    assert RR.ban_set([7], 3, eot) == set()
    assert RR.ban_set([], 1, eot) == set()
    assert RR.ban_set([4, 12, 4], 1, eot) == {4}                  # n = 1: empty suffix, every eligible id of g
    assert RR.ban_set([1, 12, 3, 1, 12], 3, eot) == {3}           # an id >= eot INSIDE the suffix matches as itself
    assert RR.ban_set([1, 2, 12, 1, 2], 3, eot) == set()          # ... and as the would-be banned id it is left alone
    assert RR.ban_set([1, 2, 3, 1, 2], 0, eot) == set()
    assert RR.seen_set([4, 12, 4, 0, 9, 10], eot) == {0, 4, 9}
    assert RR.repeated_ngrams([1, 2, 3, 1, 2, 3, 1], 3, eot) == 2
    assert RR.repeated_ngrams([1, 2, 12, 1, 2, 12], 3, eot) == 0  # the repeat ends in an id >= eot: not the rule's business
    assert RR.repeated_ngrams([7, 7, 7, 7], 2, eot) == 2
    assert RR.repeated_ngrams([1, 2, 3, 4], 1, eot) == 0 and RR.repeated_ngrams([1, 2, 1], 1, eot) == 1


def test_a_sequence_grown_under_the_ban_has_no_repeated_ngram():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 8):
        eot, g = 12, []
        for _ in range({1: 12, 2: 24}.get(n, 200)):     # (12 ids: an id has 12 successors, so 24 tokens cannot run into a dead end)
            free = [t for t in range(eot) if t not in RR.ban_set(g, n, eot)]
            g.append(int(rng.choice(free[:3])))     # (the lowest free ids: a greedy loop that the ban keeps breaking)
        assert RR.repeated_ngrams(g, n, eot) == 0, n


def test_penalty_is_one_f32_multiply():
    v = np.array([2.0, -2.0, 0.0, -0.0, 3.5, 1e-30, -7.25, 5.0], np.float32)
    for p in (1.5, 1.3, 0.5, 1.0):
        out = RR.penalise(v, {0, 1, 2, 3, 5, 6}, p)
        inv, p32 = np.float32(1.0 / float(np.float32(p))), np.float32(p)
        want = v.copy()
        for t in (0, 1, 2, 3, 5, 6):
            want[t] = v[t] * inv if v[t] > 0 else v[t] * p32
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
        assert out[4] == v[4] and out[7] == v[7]
    # against the division of Hugging Face / CTranslate2: at most one ulp
    x = np.abs(np.random.default_rng(0).standard_normal(4096).astype(np.float32)) * 9
    a, d = x * RR.inv_p(1.3), x / np.float32(1.3)
    assert np.all(np.abs(a.view(np.int32) - d.view(np.int32)) <= 1)
    row, banned = RR.apply_rules(v, [0, 1, 0, 1, 0], 1.5, 2, eot=8)
    assert np.flatnonzero(banned).tolist() == [1] and row[0] == np.float32(2.0) * RR.inv_p(1.5) and row[4] == v[4]


def test_bitmap_layout():
    assert RR.words_of(51865) == 1621 and RR.words_of(1024) == 32 and RR.words_of(1040) == 33
    w = RR.bitmap({0, 31, 32, 51864}, 51865)
    assert w[0] == 0x80000001 and w[1] == 1 and w[1620] == 1 << (51864 & 31) and int(np.count_nonzero(w)) == 3


# ---------------------------------------------------------------- the wrapper's packing
class StandIn:
    """lib.wm_set_repetition_rules records what it is handed; the wrapper sets argtypes / restype on the function"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

        def fn(*a):
            self.calls.append(a)
            return self.status
        self.wm_set_repetition_rules = fn

    def wm_last_error(self):
        return b"stand-in"


def _ctx(lib):
    c = object.__new__(B.Context)
    c.lib, c.handle = lib, ctypes.c_void_p(0x1234)
    return c


def test_the_wrapper_packs_penalty_ngram_and_eot():
    lib = StandIn()
    c = _ctx(lib)
    c.set_repetition_rules(1.5, 3, 50257)
    c.set_repetition_rules(no_repeat_ngram_size=np.int64(2), eot=np.int32(7))
    c.set_repetition_rules()
    assert [a[1:] for a in lib.calls] == [(1.5, 3, 50257), (1.0, 2, 7), (1.0, 0, 0)]
    assert all(a[0] is c.handle for a in lib.calls)
    assert all(type(a[1]) is float and type(a[2]) is int and type(a[3]) is int for a in lib.calls)
    assert lib.wm_set_repetition_rules.argtypes == [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int32]
    assert lib.wm_set_repetition_rules.restype is ctypes.c_int


def test_the_wrapper_raises_on_an_error_status():
    with pytest.raises(B.WhisperError):
        _ctx(StandIn(status=1)).set_repetition_rules(0.0, 0, 5)


# ---------------------------------------------------------------- transcribe_long on the recording fake
class RulesCtx(RecCtx):
    def set_repetition_rules(self, *a, **kw):
        self._log("set_repetition_rules", a, kw)


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def _run(case, **extra):
    ctx = RulesCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    got = dict(calls=ctx.calls)
    try:
        got["out"] = canon(B.transcribe_long(ctx, recs, **dict(case["kw"], **extra)))
    except (ValueError, RuntimeError) as e:
        got["error"] = [type(e).__name__, str(e)]
    return got


def _case_names():
    names = sorted(cases(None))
    plain = [n for n in names if not n.startswith("error_")]
    return plain[::7] + [n for n in plain if n.startswith("decode_raises")]


@pytest.mark.parametrize("name", sorted(set(_case_names())))
def test_transcribe_long_sets_the_rules_once_and_clears_them(vocab, name):
    """With the two keywords the call log is the plain run's plus ONE set call (behind the log-mel, in front of every decode)
    and ONE clear call at the very end -- also when a decode raises; with both None it is the plain run's log."""
    case = cases(vocab)[name]
    plain = run_case(case)
    none = _run(case, repetition_penalty=None, no_repeat_ngram_size=None)
    assert canon(none["calls"]) == plain["calls"]
    eot = case["kw"]["eot"]
    for kw, want in ((dict(repetition_penalty=1.5, no_repeat_ngram_size=3), [1.5, 3, eot]),
                     (dict(no_repeat_ngram_size=2), [1.0, 2, eot]), (dict(repetition_penalty=1.25), [1.25, 0, eot])):
        got = _run(case, **kw)
        assert ("error" in got) == ("error" in plain)
        if "error" in plain:
            assert got["error"] == plain["error"]
        else:
            assert got["out"] == plain["out"]
        calls = canon(got["calls"])
        at = [i for i, c in enumerate(calls) if c[0] == "set_repetition_rules"]
        assert len(at) == 2 and at[1] == len(calls) - 1, [c[0] for c in calls]
        assert calls[at[0]] == ["set_repetition_rules", want, []] and calls[at[1]] == ["set_repetition_rules", [1.0, 0, eot], []]
        assert [c for i, c in enumerate(calls) if i not in at] == plain["calls"]
        names = [c[0] for c in calls]
        mel = max(i for i, n_ in enumerate(names) if n_ in ("logmel_long", "logmel_long_device"))
        first_use = min(i for i, n_ in enumerate(names) if n_.startswith(("transcribe_", "encode_windows", "windows_detect")))
        assert mel < at[0] < first_use


def test_the_raising_case_is_among_them(vocab):
    assert any(n.startswith("decode_raises") for n in _case_names())
    got = _run(cases(vocab)["decode_raises_in_a_reuse_round"], no_repeat_ngram_size=3)
    assert got["error"][0] == "RuntimeError" and got["calls"][-1][0] == "set_repetition_rules"
