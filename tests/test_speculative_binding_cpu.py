"""CPU tests of the Python side of speculative decoding, without a device: the arguments Context.transcribe_mel_speculative
hands to wm_transcribe_mel_speculative (on the stand-in library of tests/test_binding_calls_cpu.py), transcribe_long's
draft= / draft_len= (on the recording fake context of tests/test_longform_calls_cpu.py: the ValueErrors before any library
call, the calls with a draft, and the unchanged call log with draft=None)."""
import ctypes
import importlib

import numpy as np
import pytest

import test_binding_calls_cpu as T
import test_longform_calls_cpu as L

B = importlib.import_module("openai_whisper_coreml_amd.binding")
DRAFT_HANDLE = 0xD4AF

# the new entry in the stand-in's terms, kept HERE: the other module's tables are read, never written
NAMES = "h draft blob base mel_len seek n_frames B prompts stride k max_new eot opts toks lens lp ns stats mem".split()
INS = dict(T._WIN, prompts=(T.I32, "B, stride"))
OUTS = dict(T._ONE, stats=(T.I32, "B, 4"))
FILL = dict(T.FILL, stats=3)


class SpecLib(T.FakeLib):
    """the stand-in library plus wm_transcribe_mel_speculative, recorded by the same rules"""

    def __getattr__(self, name):
        if name != "wm_transcribe_mel_speculative":
            return T.FakeLib.__getattr__(self, name)

        def fn(*args):
            assert len(args) == len(NAMES)
            d = dict(zip(NAMES, args))
            d["draft"] = None if d["draft"] is None else int(d["draft"].value)      # the draft's handle: a scalar of the record
            scal = {k: v for k, v in d.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
            rec = {}
            for k, v in d.items():
                if k == "h":
                    continue
                if v is None or k in scal:
                    rec[k] = T.plain(v)
                elif k == "opts":
                    o = v._obj
                    rec[k] = dict(temperature=T.plain(float(o.temperature)), seed=int(o.seed), no_speech_token=int(o.no_speech_token),
                                  sot_index=int(o.sot_index))
                elif k == "blob":
                    rec[k] = "device:%x" % v.value if d["mem"] == B.WM_MEM_DEVICE else T.plain(T._at(v.value, *self.blob))
                elif k in INS:
                    rec[k] = T.plain(T._at(v.value, INS[k][0], eval("(%s,)" % INS[k][1], {}, scal)))
                else:
                    dtype, shape = OUTS[k][0], eval("(%s,)" % OUTS[k][1], {}, scal)
                    rec[k] = dict(dtype=dtype, shape=list(shape))
                    T._at(v.value, dtype, shape)[...] = d["eot"] if k == "toks" else FILL[k]
            self.calls.append([name, rec])
            return B.WM_OK
        self.__dict__[name] = fn
        return fn


def _ctx(handle):
    c = T.make_ctx()
    c.lib = SpecLib()
    c.handle = ctypes.c_void_p(handle)
    return c


def test_the_wrapper_hands_the_c_function_its_arguments():
    ctx, draft = _ctx(0xC0DE), _ctx(DRAFT_HANDLE)
    ctx.lib.blob = ("float32", (48,))
    r = ctx.transcribe_mel_speculative(draft, T.MEL, T.BASE3, T.LEN3, T.SEEK3, T.NF3, T.P3, 5, 3, eot=46, no_speech_token=47,
                                       sot_index=1, budgets=[5, 2, 4])
    (n0, budgets), (n1, rec) = ctx.lib.calls
    assert n0 == "wm_set_token_budgets" and budgets["budgets"]["values"] == [5, 2, 4] and budgets["n"] == 3
    assert n1 == "wm_transcribe_mel_speculative" and draft.lib.calls == []
    assert rec["draft"] == DRAFT_HANDLE and rec["B"] == 3 and rec["stride"] == 4 and rec["k"] == 3 and rec["max_new"] == 5
    assert rec["eot"] == 46 and rec["mem"] == B.WM_MEM_HOST
    assert rec["opts"] == dict(temperature=0.0, seed=0, no_speech_token=47, sot_index=1)
    assert rec["blob"]["values"] == T.MEL.tolist() and rec["base"] == dict(dtype="int64", shape=[3], c_contiguous=True, values=T.BASE3)
    for k, want in (("mel_len", T.LEN3), ("seek", T.SEEK3), ("n_frames", T.NF3)):
        assert rec[k]["dtype"] == "int32" and rec[k]["values"] == want
    assert rec["prompts"] == dict(dtype="int32", shape=[3, 4], c_contiguous=True, values=sum(T.P3, []))
    assert rec["toks"] == dict(dtype="int32", shape=[3, 5]) and rec["lens"] == dict(dtype="int32", shape=[3])
    assert rec["lp"] == dict(dtype="float32", shape=[3, 5]) and rec["ns"] == dict(dtype="float32", shape=[3])
    assert rec["stats"] == dict(dtype="int32", shape=[3, 4])
    assert isinstance(r, B.SpeculativeResult) and isinstance(r, B.TranscribeResult)
    assert r.tokens.shape == (3, 5) and np.all(r.tokens == 46) and np.all(r.lens == 1) and np.all(r.no_speech_prob == 0.25)
    assert r.stats.shape == (3, 4) and np.all(r.stats == 3) and r.rounds.tolist() == r.kept.tolist() == [3, 3, 3]


def test_device_mel_one_prompt_for_all_and_no_no_speech_output():
    ctx, draft = _ctx(0xC0DE), _ctx(DRAFT_HANDLE)
    r = ctx.transcribe_mel_speculative(draft, T.DEV, T.BASE3, 13, 0, T.NF3, [9, 1, 2], 4, 7, mem=B.WM_MEM_DEVICE)
    (name, rec), = ctx.lib.calls
    assert rec["blob"] == "device:%x" % T.DEVICE_MEL and rec["mem"] == B.WM_MEM_DEVICE and rec["k"] == 7 and rec["eot"] == -1
    assert rec["prompts"]["values"] == [9, 1, 2] * 3 and rec["stride"] == 3 and rec["ns"] is None
    assert rec["mel_len"]["values"] == [13] * 3 and rec["seek"]["values"] == [0] * 3
    assert rec["opts"] == dict(temperature=0.0, seed=0, no_speech_token=-1, sot_index=0)
    assert r.no_speech_prob is None
    with pytest.raises(ValueError, match="prompts of one length"):
        ctx.transcribe_mel_speculative(draft, T.DEV, T.BASE3, 13, 0, T.NF3, T.RAGGED, 4, 3, mem=B.WM_MEM_DEVICE, budgets=[1, 2, 3])
    assert len(ctx.lib.calls) == 1                   # rejected before anything reached the library: no budgets left behind


# ---------------------------------------------------------------- transcribe_long
class SpecRecCtx(L.RecCtx):
    def transcribe_mel_speculative(self, *a, **kw):
        self._log("transcribe_mel_speculative", a, kw)
        self.n_spec = getattr(self, "n_spec", 0) + 1
        # the windows' scripted decodes: the rows' sample ids are what the plain call of the same rows was given
        ids = [self.spec_ids[(int(b), int(s))] for b, s in zip(a[2], a[4])]
        for b, s, sid in zip(a[2], a[4], ids):
            self.sid_of[(int(b), int(s))] = sid
        return self._decode(ids, a[7], dict(kw, temperature=0.0))


def _run(kw, ctx):
    recs = [L._rec(s) for s in L.SECONDS]
    return L.canon(B.transcribe_long(ctx, recs, **kw))


def test_draft_none_makes_exactly_the_calls_made_without_the_argument():
    for kw in (L.MIN, dict(L.STD, initial_prompt_tokens=[3, 4, 5]), dict(L.STD, initial_prompt_tokens=[[3, 4], [], [5]])):
        a, b = L.RecCtx(L.SCRIPT), L.RecCtx(L.SCRIPT)
        assert _run(kw, a) == _run(dict(kw, draft=None, draft_len=None), b)
        assert L.canon(a.calls) == L.canon(b.calls) and any(c[0] == "transcribe_mel" for c in a.calls)


def test_a_draft_takes_the_temperature_0_steps_of_uniform_rounds_and_changes_no_result():
    for kw in (L.MIN, dict(L.STD, initial_prompt_tokens=[3, 4, 5])):
        plain = L.RecCtx(L.SCRIPT)
        want = _run(kw, plain)
        draft = L.RecCtx({})
        ctx = SpecRecCtx(L.SCRIPT)
        # (base, seek) -> sample id of every window the plain run decoded
        ctx.spec_ids = dict(plain.sid_of)
        got = _run(dict(kw, draft=draft, draft_len=5), ctx)
        assert got == want
        assert [c[0] for c in draft.calls] == ["set_timestamp_rules"] and draft.calls[0][1:] == ctx.calls[0][1:]
        calls = [c for c in ctx.calls if c[0] != "set_timestamp_rules"]
        ref = [c for c in plain.calls if c[0] != "set_timestamp_rules"]
        assert len(calls) == len(ref) and ctx.n_spec >= 2
        for c, p in zip(calls, ref):
            pk = dict((k, v) for k, v in p[2])
            if p[0] == "transcribe_mel" and pk["temperature"] == 0:
                ck = dict((k, v) for k, v in c[2])
                assert c[0] == "transcribe_mel_speculative" and c[1][0] == L.canon(draft) and c[1][1:8] == p[1] and c[1][8] == 5
                assert ck == {k: v for k, v in pk.items() if k not in ("temperature", "seed", "sample_ids")}
            else:
                assert c == p      # the fallback steps above temperature 0 and everything else: unchanged
        assert any(c[0] == "transcribe_mel" for c in calls)           # a fallback step did run


def test_a_round_of_ragged_prompts_stays_on_the_plain_entry():
    kw = dict(L.STD, initial_prompt_tokens=[[3, 4], [], [5]])
    plain, ctx = L.RecCtx(L.SCRIPT), SpecRecCtx(L.SCRIPT)
    want = _run(kw, plain)
    assert _run(dict(kw, draft=L.RecCtx({}), draft_len=2), ctx) == want
    assert [c for c in ctx.calls] == [c for c in plain.calls] and not hasattr(ctx, "n_spec")


@pytest.mark.parametrize("kw, what", [
    (dict(condition_on_previous_text=True), "condition_on_previous_text"),
    (dict(best_of=2), "best_of"),
    (dict(beam_size=2), "beam_size"),
    (dict(word_timestamps="decode", vocab=object()), "word_timestamps='decode*'"),
    (dict(word_timestamps="decode_best", vocab=object(), beam_size=None), "word_timestamps='decode*'"),
    (dict(reuse_encoder=True), "reuse_encoder"),
    (dict(repetition_penalty=1.2), "the repetition rules"),
    (dict(no_repeat_ngram_size=3), "the repetition rules"),
    (dict(bad_words=[[5, 6]]), "a sequence bias"),
])
def test_combinations_that_are_not_offered_raise_before_any_library_call(kw, what):
    ctx, draft = SpecRecCtx(L.SCRIPT), L.RecCtx({})
    with pytest.raises(ValueError, match="draft \\(speculative decoding\\) cannot be combined with " + what.replace("*", "\\*")):
        B.transcribe_long(ctx, [L._rec(s) for s in L.SECONDS], **dict(L.STD, draft=draft, **kw))
    assert ctx.calls == [] and draft.calls == []


@pytest.mark.parametrize("kw, text", [
    (dict(draft_len=3), "draft_len needs draft"),
    (dict(draft=L.RecCtx({}), draft_len=0), "draft_len: 1 .. 7"),
    (dict(draft=L.RecCtx({}), draft_len=8), "draft_len: 1 .. 7"),
    (dict(draft=L.RecCtx({}), draft_len=2.5), "draft_len: 1 .. 7"),
    (dict(draft=L.RecCtx({}), draft_len=True), "draft_len: 1 .. 7"),
])
def test_draft_len_is_checked_before_any_library_call(kw, text):
    ctx = SpecRecCtx(L.SCRIPT)
    with pytest.raises(ValueError, match=text):
        B.transcribe_long(ctx, [L._rec(s) for s in L.SECONDS], **dict(L.STD, **kw))
    assert ctx.calls == []


def test_the_default_draft_len():
    ctx, plain = SpecRecCtx(L.SCRIPT), L.RecCtx(L.SCRIPT)
    _run(L.MIN, plain)
    ctx.spec_ids = dict(plain.sid_of)
    _run(dict(L.MIN, draft=L.RecCtx({})), ctx)
    assert {c[1][8] for c in ctx.calls if c[0] == "transcribe_mel_speculative"} == {4}
