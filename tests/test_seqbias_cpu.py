"""The sequence bias (wm_set_sequence_bias) without a device: the numpy restatement (tests/seqbias_ref.py)
against a brute-force enumeration and against Hugging Face's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor, the
wrapper's packing against a stand-in library, and transcribe_long's calls on the recording fake of
test_longform_calls_cpu.py."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import seqbias_ref as SB
from test_longform_calls_cpu import RecCtx, cases, make_vocab, run_case, canon
from test_longform_clips_cpu import _rec
from test_longform_calls_cpu import SECONDS

B = importlib.import_module("openai_whisper_coreml_amd.binding")
INF = math.inf


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the restatement against a brute force
def brute_row(v, table, g):
    """By the meaning of the rule, id by id: append t to the history and look at every entry that the extended history ENDS
    in; sum their biases in table order, in float32, starting from +0.0."""
    g = [int(t) for t in g]
    out, banned = np.array(v, np.float32), np.zeros(len(v), bool)
    for t in range(len(v)):
        h = g + [t]
        total = np.float32(0.0)
        for s, b in table:
            if len(h) >= len(s) and tuple(h[len(h) - len(s):]) == tuple(s):
                total = np.float32(total + np.float32(b))
        with np.errstate(invalid="ignore"):
            out[t] = np.float32(out[t] + total)
        banned[t] = total == -np.inf
    return out, banned


def histories(rng, k, V, s):
    """histories of k tokens: random, and ones that END in the context of s (so that the entry matches when k allows)"""
    yield "random", rng.integers(0, V, k)
    yield "few ids", rng.integers(0, 3, k)
    ctx = list(s[:-1])
    if k >= len(ctx):
        yield "ends in the context", np.concatenate([rng.integers(0, V, k - len(ctx)), ctx]).astype(np.int64)
    if k >= 1 and ctx:
        h = np.concatenate([rng.integers(0, V, k), ctx])[-k:].astype(np.int64)
        yield "ends in the context, cut to k", h
        h2 = h.copy()
        h2[-1] = (h2[-1] + 1) % V
        yield "the newest token differs", h2
        h3 = h.copy()
        h3[0 if k < len(ctx) else k - len(ctx)] = (h3[0 if k < len(ctx) else k - len(ctx)] + 1) % V
        yield "the oldest context token differs", h3


@pytest.mark.parametrize("n", [1, 2, 3, 32])
def test_the_restatement_against_the_brute_force(n):
    V, eot = 24, 20                                   # ids 20 .. 23 never end an entry but stand inside one and in the history
    rng = np.random.default_rng(200 + n)
    v = rng.standard_normal(V).astype(np.float32) * 3
    v[3] = np.float32(-0.0)
    main = tuple(int(t) for t in rng.integers(0, eot, n))
    inner = main if n < 3 else main[:1] + (eot + 1,) + main[2:]       # an id >= eot INSIDE the sequence
    last = inner[-1]
    other = tuple((t + 1) % eot for t in inner[:-1]) + (last,)
    seqs = [inner, (last,) if n > 1 else ((last + 1) % eot,), (5, 7), (9, 7), (7,), (6, 5, 7)]
    bias = [1.25, 0.1, 0.3, -INF, 1e-3, 7.0]
    if n > 1 and other != inner:
        seqs.append(other)
        bias.append(-2.5)
    seqs2, bias2 = [], []
    for s, b in zip(seqs, bias):                       # (drop accidental duplicates of the random sequence)
        if s not in seqs2:
            seqs2.append(s)
            bias2.append(b)
    table = SB.expand(seqs2, bias2, eot=eot, V=V)
    for k in sorted({0, max(n - 2, 0), n - 1, n, 447}):
        for name, g in histories(rng, k, V, inner):
            got, banned = SB.apply_bias(v, table, g)
            want, wbanned = brute_row(v, table, g)
            assert np.array_equal(bits(got), bits(want)), (n, k, name)
            assert np.array_equal(banned, wbanned), (n, k, name)
            if name == "ends in the context" or (n == 1):
                assert SB.matches(inner, g)
            if k < n - 1:
                assert not SB.matches(inner, g)


def test_hand_made_tables():
    eot, V = 10, 12
    v = np.arange(V, dtype=np.float32)
    # several entries on one last token: the sum runs in TABLE order, in float32 -- 1e8 + 1 - 1e8 is 0, not 1
    t = SB.expand([(1, 7), (7,), (2, 1, 7)], [1e8, 1.0, -1e8], eot=eot, V=V)
    assert SB.totals(t, [2, 1]) == {7: np.float32(np.float32(np.float32(1e8) + np.float32(1.0)) + np.float32(-1e8))}
    assert SB.totals(t, [2, 1])[7] == 0.0 and SB.totals(t, [3, 1])[7] == np.float32(1e8) + np.float32(1.0)
    t2 = SB.expand([(7,), (2, 1, 7), (1, 7)], [1.0, -1e8, 1e8], eot=eot, V=V)
    assert SB.totals(t2, [2, 1])[7] == 0.0 + np.float32(np.float32(np.float32(1.0) + np.float32(-1e8)) + np.float32(1e8))
    assert SB.totals(t, []) == {7: np.float32(1.0)} and SB.totals(t, [1]) == {7: np.float32(np.float32(1e8) + np.float32(1.0))}
    # an id >= eot inside a sequence matches as itself; as a last token it is refused
    t = SB.expand([(11, 3)], [2.0], eot=eot, V=V)
    assert SB.totals(t, [5, 11]) == {3: np.float32(2.0)} and SB.totals(t, [11, 5]) == {}
    with pytest.raises(SB.Invalid):
        SB.expand([(3, 11)], [2.0], eot=eot, V=V)
    # -inf plus a finite bias on one id: a ban whatever the order; the finite entry alone is a bias
    for seqs, bias in (([(4,), (1, 4)], [3.0, -INF]), ([(1, 4), (4,)], [-INF, 3.0])):
        t = SB.expand(seqs, bias, eot=eot, V=V)
        row, banned = SB.apply_bias(v, t, [1])
        assert banned.tolist() == [i == 4 for i in range(V)] and row[4] == -np.inf
        row, banned = SB.apply_bias(v, t, [2])
        assert not banned.any() and row[4] == np.float32(7.0)
    # v + 0.0 for every id: -0.0 becomes +0.0, as in Hugging Face (scores + bias)
    row, _ = SB.apply_bias(np.array([-0.0, 1.0], np.float32), SB.expand([(1,)], [0.5], eot=2, V=2), [])
    assert bits(row).tolist() == [0, bits(np.float32(1.5))[()]]


def test_prefix_expansion():
    eot, V = 100, 120
    # a boosted phrase: itself, then its proper prefixes, shortest first, all with its bias
    assert SB.expand([(1, 2, 3)], [2.0], [True], eot=eot, V=V) == [((1, 2, 3), 2.0), ((1,), 2.0), ((1, 2), 2.0)]
    assert SB.expand([(1, 2, 3)], [2.0], [False], eot=eot, V=V) == [((1, 2, 3), 2.0)]
    # shared first tokens merge into the FIRST implicit entry with the MAXIMUM bias: boosted once, as a trie would
    t = SB.expand([(1, 2, 3), (1, 2, 4), (1, 5)], [2.0, 3.0, 1.0], [True, True, True], eot=eot, V=V)
    assert t == [((1, 2, 3), 2.0), ((1,), 3.0), ((1, 2), 3.0), ((1, 2, 4), 3.0), ((1, 5), 1.0)]
    assert SB.totals(t, []) == {1: np.float32(3.0)} and SB.totals(t, [1]) == {1: np.float32(3.0), 2: np.float32(3.0), 5: np.float32(1.0)}
    # an implicit entry identical to a GIVEN sequence is dropped, wherever the given one stands
    t = SB.expand([(1, 2, 3), (1, 2)], [2.0, -0.5], [True, False], eot=eot, V=V)
    assert t == [((1, 2, 3), 2.0), ((1,), 2.0), ((1, 2), -0.5)]
    t = SB.expand([(1, 2), (1, 2, 3)], [-INF, 2.0], [False, True], eot=eot, V=V)
    assert t == [((1, 2), -INF), ((1, 2, 3), 2.0), ((1,), 2.0)]
    # a prefix that ends in an id >= eot gives no entry (only text ids are ever biased); the longer ones stay
    t = SB.expand([(1, 110, 3)], [2.0], [True], eot=eot, V=V)
    assert t == [((1, 110, 3), 2.0), ((1,), 2.0)]
    # -inf cannot boost its prefixes
    with pytest.raises(SB.Invalid):
        SB.expand([(1, 2)], [-INF], [True], eot=eot, V=V)
    # the limit counts the entries AFTER expansion and merge
    seqs = [(i // 100, 50 + i % 50, i % 100) for i in range(1365)]          # 1365 distinct 3-token phrases
    assert len(set(seqs)) == 1365
    n = len(SB.expand(seqs, [1.0] * 1365, [True] * 1365, eot=eot, V=V))
    assert n == 1365 + len({s[:1] for s in seqs}) + len({s[:2] for s in seqs}) <= SB.MAX_ENTRIES
    ok = [(i,) for i in range(96)] + [(a, b) for a in range(40) for b in range(100)]
    assert len(SB.expand(ok, [1.0] * len(ok), eot=eot, V=V)) == 4096
    with pytest.raises(SB.Invalid):
        SB.expand(ok + [(96,)], [1.0] * (len(ok) + 1), eot=eot, V=V)
    many = [(a, 10 + b, c) for a in range(10) for b in range(20) for c in range(20)]   # 4000 given + 10 + 200 implicit
    with pytest.raises(SB.Invalid):
        SB.expand(many, [1.0] * 4000, [True] * 4000, eot=eot, V=V)
    assert len(SB.expand(many, [1.0] * 4000, [False] * 4000, eot=eot, V=V)) == 4000


def test_invalid_tables():
    eot, V = 10, 12
    for seqs, bias, boost in (([(12,)], [1.0], None), ([(-1, 2)], [1.0], None), ([(1, 10)], [1.0], None), ([()], [1.0], None),
                              ([tuple([1] * 33)], [1.0], None), ([(1,)], [math.nan], None), ([(1,)], [INF], None),
                              ([(1, 2), (1, 2)], [1.0, 2.0], None), ([(1, 2)], [-INF], [True])):
        with pytest.raises(SB.Invalid):
            SB.expand(seqs, bias, boost, eot=eot, V=V)
    for eot_ in (-1, V + 1):
        with pytest.raises(SB.Invalid):
            SB.expand([(1,)], [1.0], eot=eot_, V=V)
    assert len(SB.expand([tuple([1] * 32)], [-INF], eot=eot, V=V)) == 1 and SB.expand([], [], eot=0, V=V) == []


# ---------------------------------------------------------------- Hugging Face's processors, bit for bit
def _hf_ids(g, start):
    """Hugging Face hands a processor the decoder sequence, which begins with the decoder start token: one id in front of the
    generated history (it stands in no entry here; a match reads the newest n - 1 tokens only).  With it Hugging Face's
    `len(sequence) > input_ids.shape[1]: ignore` is this project's `k >= n - 1`."""
    torch = pytest.importorskip("torch")
    return torch.tensor([[start] + [int(t) for t in g]], dtype=torch.long)


def test_bit_for_bit_hugging_face_sequence_bias_and_bad_words():
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    V, eot = 64, 60
    rng = np.random.default_rng(7)
    # Hugging Face adds the single-token biases first, then the longer sequences in dict order: the same order here
    seqs = [(5,), (9,), (3, 5), (4, 3, 5), (8, 9), (1, 2, 3, 4, 6), (7, 9), (61, 9), (2, 2)]
    bias = [0.1, -0.7, 1e8, -1e8, 0.3, 2.5, 1.7, -3.0, 0.25]
    table = SB.expand(seqs, bias, eot=eot, V=V)
    hf = lp.SequenceBiasLogitsProcessor(sequence_bias={s: float(np.float32(b)) for s, b in zip(seqs, bias)})
    bad = [(3, 5), (9,), (1, 2, 3, 4, 6), (61, 9)]
    btable = SB.expand(bad, [-INF] * len(bad), eot=eot, V=V)
    hfb = lp.NoBadWordsLogitsProcessor(bad_words_ids=[list(s) for s in bad])
    n_hist = 0
    for k in (0, 1, 2, 3, 4, 5, 30):
        for tail in ([], [3], [4, 3], [8], [1, 2, 3, 4], [7], [61], [2], [3, 5]):
            if len(tail) > k:
                continue
            g = np.concatenate([rng.integers(0, V, k - len(tail)), tail]).astype(np.int64)
            v = (rng.standard_normal(V) * 4).astype(np.float32)
            want = hf(_hf_ids(g, V - 1), torch.from_numpy(v.copy())[None])[0].numpy()
            got, banned = SB.apply_bias(v, table, g)
            assert np.array_equal(bits(got), bits(want)), (k, tail)
            assert not banned.any()
            want = hfb(_hf_ids(g, V - 1), torch.from_numpy(v.copy())[None])[0].numpy()
            got, banned = SB.apply_bias(v, btable, g)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(banned, want == -np.inf), (k, tail)
            n_hist += 1
    assert n_hist > 40


# ---------------------------------------------------------------- the wrapper's packing
class StandIn:
    """lib.wm_set_sequence_bias records what it is handed (arrays copied out of the pointers)"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

        def fn(handle, toks, offs, bias, flags, n, eot):
            def read(p, ct, count):
                return None if p is None else list(ctypes.cast(p, ctypes.POINTER(ct))[:count])
            o = read(offs, ctypes.c_int32, n + 1)
            self.calls.append((handle, read(toks, ctypes.c_int32, o[-1] if o else 0), o, read(bias, ctypes.c_float, n),
                               read(flags, ctypes.c_uint8, n), n, eot))
            return self.status
        self.wm_set_sequence_bias = fn

    def wm_last_error(self):
        return b"stand-in"


def _ctx(lib):
    c = object.__new__(B.Context)
    c.lib, c.handle, c.dims = lib, ctypes.c_void_p(0x1234), dict(n_vocab=51865)
    return c


def test_the_wrapper_packs_the_table():
    lib = StandIn()
    c = _ctx(lib)
    c.set_sequence_bias({(5, 6, 7): 2.0, (np.int64(9),): -INF, (1, 2): 0.5}, boost=[(1, 2), (5, 6, 7)], eot=50257)
    c.set_sequence_bias({(3,): 1.5})
    c.set_sequence_bias(None)
    c.set_sequence_bias({}, eot=7)
    assert lib.calls[0][1:] == ([5, 6, 7, 9, 1, 2], [0, 3, 4, 6], [2.0, -INF, 0.5], [1, 0, 1], 3, 50257)
    assert lib.calls[1][1:] == ([3], [0, 1], [1.5], None, 1, 51865)
    assert lib.calls[2][1:] == (None, None, None, None, 0, 51865) and lib.calls[3][1:] == (None, None, None, None, 0, 7)
    assert all(a[0] is c.handle and type(a[5]) is int and type(a[6]) is int for a in lib.calls)
    assert lib.wm_set_sequence_bias.argtypes == [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int32]
    assert lib.wm_set_sequence_bias.restype is ctypes.c_int
    with pytest.raises(ValueError):
        c.set_sequence_bias({(1, 2): 1.0}, boost=[(1, 3)])
    # the packing is what the restatement's pack() gives the C call
    toks, offs, bias, flags = SB.pack([(5, 6, 7), (9,), (1, 2)], [2.0, -INF, 0.5], [True, False, True])
    assert (toks.tolist(), offs.tolist(), bias.tolist(), flags.tolist()) == lib.calls[0][1:5]


def test_the_wrapper_raises_on_an_error_status():
    with pytest.raises(B.WhisperError):
        _ctx(StandIn(status=1)).set_sequence_bias({(1,): 1.0})


def test_long_bias_table():
    f = B.long_bias_table
    assert f(None, None, None, None) is None
    assert f({(1, 2): 0.5}, [[3, 4], (5,)], [[6, 7, 8]], 2.0) == ({(1, 2): 0.5, (3, 4): -INF, (5,): -INF, (6, 7, 8): 2.0}, [(6, 7, 8)])
    assert list(f({(1, 2): 0.5}, [[3, 4]], [[6, 7]], 2.0)[0]) == [(1, 2), (3, 4), (6, 7)]          # the order of the table
    assert f(None, [], None, None) == ({}, [])
    for args in (({(1, 2): 0.5}, [[1, 2]], None, None), (None, [[1]], [[1]], 1.0), (None, None, [[1, 2]], None), (None, None, [[1, 2]], INF)):
        with pytest.raises(ValueError):
            f(*args)


# ---------------------------------------------------------------- transcribe_long on the recording fake
class BiasCtx(RecCtx):
    def set_sequence_bias(self, sequences=None, boost=(), eot=None):
        self.calls.append(["set_sequence_bias", None if sequences is None else [[list(k), v] for k, v in sequences.items()],
                           [list(k) for k in boost], eot])

    def set_repetition_rules(self, *a, **kw):
        self._log("set_repetition_rules", a, kw)


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def _run(case, **extra):
    ctx = BiasCtx(case["script"], **case.get("ctx", {}))
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
def test_transcribe_long_sets_the_table_once_and_clears_it(vocab, name):
    """With the options the call log is the plain run's plus ONE set call (behind the log-mel, in front of every decode) and ONE
    clear call at the very end -- also when a decode raises; with all of them None it is the plain run's log."""
    case = cases(vocab)[name]
    plain = run_case(case)
    none = _run(case, sequence_bias=None, bad_words=None, boost_phrases=None, phrase_boost=None)
    assert canon(none["calls"]) == plain["calls"]
    eot = case["kw"]["eot"]
    for kw, want in ((dict(sequence_bias={(1, 2): 0.5, (3,): -1.0}), [[[1, 2], 0.5], [[3], -1.0]]),
                     (dict(bad_words=[[4, 5], [6]]), [[[4, 5], -INF], [[6], -INF]]),
                     (dict(sequence_bias={(1, 2): 0.5}, bad_words=[[4, 5]], boost_phrases=[[7, 8, 9]], phrase_boost=2.0),
                      [[[1, 2], 0.5], [[4, 5], -INF], [[7, 8, 9], 2.0]])):
        got = _run(case, **kw)
        assert ("error" in got) == ("error" in plain)
        if "error" in plain:
            assert got["error"] == plain["error"]
        else:
            assert got["out"] == plain["out"]
        calls = got["calls"]
        at = [i for i, c in enumerate(calls) if c[0] == "set_sequence_bias"]
        assert len(at) == 2 and at[1] == len(calls) - 1, [c[0] for c in calls]
        boost = [[7, 8, 9]] if "boost_phrases" in kw else []
        assert calls[at[0]] == ["set_sequence_bias", want, boost, eot] and calls[at[1]] == ["set_sequence_bias", None, [], None]
        assert canon([c for i, c in enumerate(calls) if i not in at]) == plain["calls"]
        names = [c[0] for c in calls]
        mel = max(i for i, n_ in enumerate(names) if n_ in ("logmel_long", "logmel_long_device"))
        first_use = min(i for i, n_ in enumerate(names) if n_.startswith(("transcribe_", "encode_windows", "windows_detect")))
        assert mel < at[0] < first_use


def test_the_raising_case_and_both_rule_sets(vocab):
    assert any(n.startswith("decode_raises") for n in _case_names())
    got = _run(cases(vocab)["decode_raises_in_a_reuse_round"], bad_words=[[4, 5]], no_repeat_ngram_size=3)
    assert got["error"][0] == "RuntimeError"
    assert [c[0] for c in got["calls"][-2:]] == ["set_sequence_bias", "set_repetition_rules"]
    names = [c[0] for c in got["calls"]]
    assert names.count("set_sequence_bias") == 2 and names.index("set_repetition_rules") < names.index("set_sequence_bias")
    # a sequence named twice is refused before any library call
    bad = _run(cases(vocab)["decode_raises_in_a_reuse_round"], bad_words=[[4, 5]], sequence_bias={(4, 5): 1.0})
    assert bad["error"][0] == "ValueError" and bad["calls"] == []
