"""The constraint (wm_set_constraint) without a device: tests/constraint_ref.py held to brute force, to
transformers' PrefixConstrainedLogitsProcessor where it imports, the builders of the binding held to the restatement, the
wrappers' packing on a stand-in library, transcribe_long's call log and the ValueErrors."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import constraint_ref as CR
import test_longform_calls_cpu as LC

B = importlib.import_module("openai_whisper_coreml_amd.binding")

EOT, V = 6, 12                     # an alphabet of 6 text ids; eot 6; 7 .. 11 stand for timestamps and specials
ALPHA = list(range(EOT))
CHOICES = [(1, 2), (1, 3, 4), (5,), (0, 0, 0, 0, 1), (1, 2, 2)]


def strings(max_len):
    for n in range(max_len + 1):
        yield from itertools.product(ALPHA, repeat=n)


def members(a, start, max_len=5):
    """the strings up to max_len the automaton ACCEPTS read as a recogniser (no use of allowed()): fold, then accept"""
    out = set()
    for w in strings(max_len):
        s = CR.fold(a, start, w)
        if s != CR.DEAD and a.accept[s]:
            out.add(w)
    return out


def anything_but():
    """state 0: any id but 2 and 4 -> state 1; state 1: exactly id 3 -> accepting state 2"""
    return CR.Automaton([0, 2, 3, 3], [2, 4, 3], [-1, -1, 2], [1, -1, -1], [0, 0, 1], EOT)


def free_text():
    """`5` then free text: state 0 -5-> 1; state 1 loops on anything and accepts"""
    return CR.Automaton([0, 1, 1], [5], [1], [-1, 1], [0, 1], EOT)


LANGS = {
    "choices": lambda: (CR.from_choices(CHOICES, EOT), set(CHOICES)),
    "repeat": lambda: (CR.from_choices(CHOICES[:3], EOT, repeat=True),
                       {w for n in range(6) for parts in itertools.product(CHOICES[:3], repeat=n)
                        for w in [tuple(t for p in parts for t in p)] if len(w) <= 5}),
    "anything but": lambda: (anything_but(), {(t, 3) for t in ALPHA if t not in (2, 4)}),
    "free text": lambda: (free_text(), {(5,) + w for w in strings(4)}),
}


@pytest.mark.parametrize("name", sorted(LANGS))
def test_the_generated_strings_are_exactly_the_language(name):
    """Alphabet of 6 ids, every string up to length 5: what always choosing an allowed id and ending at an allowed eot can
    produce == what the automaton accepts as a recogniser == the language written down by hand."""
    a, want = LANGS[name]()
    assert CR.invalid(a, V) is None
    assert CR.language(a, 0, ALPHA, 5) == want
    assert members(a, 0) == want
    # a prefix of a member never reaches the dead state, a string that is no prefix of a member does
    prefixes = {w[:i] for w in CR.language(a, 0, ALPHA, 6) for i in range(len(w) + 1)}
    for w in strings(4):
        assert (CR.fold(a, 0, w) != CR.DEAD) == (w in prefixes), w


def test_transparent_ids_and_the_dead_state():
    a = CR.from_choices(CHOICES, EOT)
    s = CR.fold(a, 0, [1])
    assert CR.fold(a, 0, [7, 1, 11, 9]) == s and CR.fold(a, 0, [1, EOT, EOT]) == s       # ids > eot and the padding eot do not move it
    assert CR.delta(a, s, 8) == s and CR.delta(a, s, EOT) == s
    assert CR.fold(a, 0, [1, 5]) == CR.DEAD and CR.fold(a, 0, [1, 5, 1, 2, 9]) == CR.DEAD  # dead stays dead
    ok = CR.allowed(a, CR.DEAD)
    assert ok[EOT] and not ok[:EOT].any()
    # the ban words: nothing above eot is ever set, incoming bits survive, a row on -1 keeps its words
    words = CR.words_of(V)
    ban_in = np.zeros(words, np.uint32)
    ban_in[0] = (1 << 0) | (1 << 9)
    out, st = CR.ban_words(a, 0, [1], ban_in)
    assert st == s and int(out[0]) == ((1 << 0) | (1 << 9) | sum(1 << t for t in range(EOT + 1) if t not in (2, 3)))
    out, st = CR.ban_words(a, -1, [1], ban_in)
    assert st is None and np.array_equal(out, ban_in)
    assert not CR.banned_mask(a, 0, [1, 5], V)[EOT:].any() and CR.banned_mask(a, 0, [1, 5], V)[:EOT].all()


BAD = {
    "offsets": [dict(edge_beg=[1, 2, 3, 3]), dict(edge_beg=[0, 2, 1, 3])],
    "ascending": [dict(edge_tok=[4, 2, 3]), dict(edge_tok=[2, 2, 3])],
    "edge token": [dict(edge_tok=[2, EOT, 3]), dict(edge_tok=[-1, 4, 3])],
    "edge_next": [dict(edge_next=[-1, -1, 3]), dict(edge_next=[-2, -1, 2])],
    "def_next": [dict(def_next=[3, -1, -1]), dict(def_next=[1, -2, -1])],
    "explicit -1": [dict(def_next=[-1, -1, -1], edge_next=[-1, 1, 2])],
    "stuck": [dict(accept=[0, 0, 0]), dict(edge_beg=[0, 2, 2, 2], accept=[0, 0, 1])],
    "eot": [dict(eot=V), dict(eot=-1)],
}


def variant(**kw):
    base = dict(edge_beg=[0, 2, 3, 3], edge_tok=[2, 4, 3], edge_next=[-1, -1, 2], def_next=[1, -1, -1], accept=[0, 0, 1], eot=EOT)
    base.update(kw)
    return CR.Automaton(**base)


@pytest.mark.parametrize("rule", sorted(BAD))
def test_every_rejected_table(rule):
    assert CR.invalid(variant(), V) is None
    for kw in BAD[rule]:
        assert CR.invalid(variant(**kw), V) == rule, kw
    big = CR.Automaton([0] + [0] * (CR.MAX_STATES + 1), [], [], [0] * (CR.MAX_STATES + 1), [1] * (CR.MAX_STATES + 1), EOT)
    assert CR.invalid(big, V) == "states"


def test_against_transformers_prefix_constrained_processor():
    """PrefixConstrainedLogitsProcessor driven by a prefix_allowed_tokens_fn read off the same automaton masks exactly the ids
    <= eot the restatement bans."""
    transformers = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    for name in sorted(LANGS):
        a, _ = LANGS[name]()
        hists = [[], [1], [1, 2], [5, 0, 3], [7, 1, 9], [1, 5, 1], [0, 3], [3, 3]]

        def fn(batch_id, ids):
            ok = CR.allowed(a, CR.fold(a, 0, [int(t) for t in ids]))
            return [int(t) for t in np.flatnonzero(ok)] + list(range(EOT + 1, V))      # ids above eot: never the constraint's
        proc = transformers.PrefixConstrainedLogitsProcessor(fn, num_beams=1)
        for h in hists:
            scores = torch.tensor(rng.standard_normal((1, V)), dtype=torch.float32)
            out = proc(torch.tensor([h], dtype=torch.long).reshape(1, len(h)), scores.clone())
            masked = np.asarray(torch.isinf(out[0]) & (out[0] < 0))
            assert np.array_equal(masked, CR.banned_mask(a, 0, h, V)), (name, h)
            assert torch.equal(out[0][~torch.as_tensor(masked)], scores[0][~torch.as_tensor(masked)])


# ------------------------------------------------------------------ the binding's builders
def test_the_builders_equal_the_restatement():
    for repeat, ch in ((False, CHOICES), (True, CHOICES[:3])):
        got = CR.of_binding(B.constraint_from_choices(ch, repeat=repeat), EOT)
        want = CR.from_choices(ch, EOT, repeat=repeat)
        assert CR.invalid(got, V) is None
        assert CR.language(got, 0, ALPHA, 5) == CR.language(want, 0, ALPHA, 5) == LANGS["repeat" if repeat else "choices"]()[1]
    parts = [B.constraint_from_choices(CHOICES), B.constraint_from_choices([(2,), (3, 3)], repeat=True),
             B.Constraint(*free_text().arrays()[:1], free_text().edge_tok, free_text().edge_next, free_text().def_next, free_text().accept)]
    joined, starts = B.constraint_join(parts)
    ref, rstarts = CR.join([CR.of_binding(p, EOT) for p in parts])
    assert starts == rstarts == [0, parts[0].n_states, parts[0].n_states + parts[1].n_states]
    j = CR.of_binding(joined, EOT)
    assert CR.invalid(j, V) is None
    for p, s in zip(parts, starts):      # a sub-automaton from its start is the automaton alone: the parts are disjoint
        assert CR.language(j, s, ALPHA, 5) == CR.language(CR.of_binding(p, EOT), 0, ALPHA, 5) == CR.language(ref, s, ALPHA, 5)


def test_the_builders_value_errors():
    for bad in ([], [[]], [[1], []], [[1, -2]]):
        with pytest.raises(ValueError):
            B.constraint_from_choices(bad)
    with pytest.raises(ValueError):
        B.constraint_from_choices([[1], [1, 2]], repeat=True)
    with pytest.raises(ValueError):
        B.constraint_from_choices([[i, j, 0] for i in range(70) for j in range(70)])       # 4971 states
    with pytest.raises(ValueError):
        B.constraint_join([])
    with pytest.raises(ValueError):
        B.constraint_join([B.constraint_from_choices([[1]]), "x"])
    with pytest.raises(ValueError):
        B.Constraint([0, 1], [1, 2], [0, 0], [-1], [1])
    a = B.constraint_from_choices(CHOICES)
    for kw in (dict(constraint="x"), dict(constraint=None, constraint_rows=[0]), dict(constraint=a, constraint_rows=[0, a.n_states]),
               dict(constraint=a, constraint_rows=[0, -2]), dict(constraint=a, constraint_rows=[0], rows=2)):
        with pytest.raises(ValueError):
            B.constraint_args(**kw)
    assert B.constraint_args(a, [0, None, 3], 3) == [0, -1, 3] and B.constraint_args(a) is None and B.constraint_args(None) is None


# ------------------------------------------------------------------ the wrappers' packing
class FakeFn:
    def __init__(self, log, name):
        self.log, self.name, self.argtypes, self.restype = log, name, None, None

    def __call__(self, *args):
        self.log.append((self.name, args, list(self.argtypes)))
        return 0


class FakeLib:
    def __init__(self):
        self.log = []
        self.wm_set_constraint = FakeFn(self.log, "wm_set_constraint")
        self.wm_set_constraint_rows = FakeFn(self.log, "wm_set_constraint_rows")


def at(p, dtype, n):
    return np.frombuffer((ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(p.value), dtype=dtype).copy()


def test_the_wrappers_packing_on_a_stand_in_library():
    ctx = object.__new__(B.Context)
    ctx.lib, ctx.handle, ctx.dims = FakeLib(), 77, dict(n_vocab=V)
    a = B.constraint_from_choices(CHOICES)
    ctx.set_constraint(a, eot=EOT)
    ctx.set_constraint(a)
    ctx.set_constraint(None)
    ctx.set_constraint_rows([0, None, 3])
    ctx.set_constraint_rows([])
    vp = ctypes.c_void_p
    (n0, a0, t0), (_, a1, _), (_, a2, _), (n3, a3, t3), (_, a4, _) = ctx.lib.log
    assert n0 == "wm_set_constraint" and t0 == [vp] * 6 + [ctypes.c_int, ctypes.c_int32]
    S, E = a.n_states, a.n_edges
    assert a0[0] == 77 and a0[6:] == (S, EOT) and a1[6:] == (S, V - 1)
    assert np.array_equal(at(a0[1], np.int32, S + 1), a.edge_beg) and np.array_equal(at(a0[2], np.int32, E), a.edge_tok)
    assert np.array_equal(at(a0[3], np.int32, E), a.edge_next) and np.array_equal(at(a0[4], np.int32, S), a.def_next)
    assert np.array_equal(at(a0[5], np.uint8, S), a.accept)
    assert a2 == (77, None, None, None, None, None, 0, 0)
    assert n3 == "wm_set_constraint_rows" and t3 == [vp, vp, ctypes.c_int]
    assert a3[0] == 77 and a3[2] == 3 and np.array_equal(at(a3[1], np.int32, 3), [0, -1, 3])
    assert a4 == (77, None, 0)
    one = B.Constraint([0, 0], [], [], [0], [1])            # no explicit edge: null edge pointers
    ctx.set_constraint(one, eot=EOT)
    assert ctx.lib.log[-1][1][2] is None and ctx.lib.log[-1][1][3] is None
    with pytest.raises(ValueError):
        ctx.set_constraint("x")


# ------------------------------------------------------------------ transcribe_long's call log
class CstCtx(LC.RecCtx):
    def set_constraint(self, *a, **kw):
        self._log("set_constraint", [type(x).__name__ if x is not None else None for x in a], kw)


def long_calls(case, **extra):
    ctx = CstCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [LC._rec(s) for s in LC.SECONDS]
    err = None
    try:
        B.transcribe_long(ctx, recs, **dict(case["kw"], **extra))
    except (ValueError, RuntimeError) as e:
        err = type(e).__name__
    return ctx.calls, err


@pytest.mark.parametrize("name", ["defaults", "reuse_best_of", "words", "decode_raises_in_a_reuse_round"])
def test_transcribe_long_makes_the_plain_calls_plus_one_set_and_one_clear(name, tmp_path):
    vocab = LC.make_vocab(tmp_path)
    try:
        case = LC.cases(vocab)[name]
        plain, err0 = long_calls(case)
        got, err1 = long_calls(case, constraint=B.constraint_from_choices(CHOICES))
        assert err0 == err1 == ("RuntimeError" if name.startswith("decode_raises") else None)
        extra = [c for c in got if c[0] == "set_constraint"]
        assert [c for c in got if c[0] != "set_constraint"] == plain
        eot = case["kw"]["eot"]
        assert extra == [["set_constraint", ["Constraint"], [["eot", eot]]], ["set_constraint", [None], []]]
        i_set, i_clear = got.index(extra[0]), got.index(extra[1])
        first_decode = min(i for i, c in enumerate(got) if c[0] in ("transcribe_mel", "transcribe_windows", "encode_windows"))
        # set in front of the first decode; cleared on leaving, behind the last decode and the mel's release (only the clearing
        # of rules set earlier may follow)
        assert i_set < first_decode < i_clear and got[i_clear - 1][0] == "dev_free"
        assert all(c[0].startswith("set_") for c in got[i_clear + 1:])
        # a bad value raises before ANY library call
        for bad in (dict(constraint="x"), dict(constraint=B.constraint_from_choices(CHOICES), draft=object())):
            calls, err = long_calls(case, **bad)
            assert err == "ValueError" and calls == []
    finally:
        vocab.close()
