"""CPU tests of window sets: the rounds of binding.transcribe_long(reuse_encoder=True) on a recording fake context -- one
encode per round, every fallback step decoding its own `todo` rows of that set, the word step aligning the kept rows, the
set freed whatever happens -- and the ctypes mirror of the new C ABI against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_longform_words_cpu import B, EOT, LANG_EN, LANG_ZH, NO_TS, SCRIPT, FakeCtx, _fake_kw, vocab  # noqa: F401  (vocab: fixture)


class FakeSet:
    def __init__(self, owner, base, seek, n_frames):
        self.owner, self.base, self.seek, self.n_frames = owner, base, seek, n_frames
        self.closed = 0
        self.decodes = []   # (temperature, rows) of every call that read it
        self.aligns = []    # rows of every align call

    def close(self):
        self.closed += 1


class FakeSetCtx(FakeCtx):
    """FakeCtx whose windows can be encoded into a FakeSet.  Recording 0 is `hard`: below `easy_from` its decode is bad
    enough (avg_logprob -5) to need the next fallback temperature.  fail_at: the n-th decode from a set raises."""

    def __init__(self, script, easy_from=0.4, fail_at=None):
        super().__init__(script)
        self.sets, self.easy_from, self.fail_at = [], easy_from, fail_at
        self.n_decodes = 0
        self.mel_calls = 0
        self.by_base = {}

    def encode_windows(self, mel, mel_base, mel_len, seek, n_frames, mem=0):
        assert mem == B.WM_MEM_DEVICE
        s = FakeSet(self, [int(b) for b in mel_base], [int(x) for x in seek], [int(n) for n in n_frames])
        self.sets.append(s)
        return s

    def transcribe_mel(self, *a, **kw):
        self.mel_calls += 1
        r = super().transcribe_mel(*a, **kw)
        # (a fallback step decodes a part of the round's rows: the align fake looks rows up among ALL of them)
        self.by_base.update(zip(self.round_base, self.round_ids))
        self.round_base, self.round_ids = list(self.by_base), list(self.by_base.values())
        t = kw.get("temperature", 0.0)
        for i, sid in enumerate(kw["sample_ids"]):
            if int(sid) & 0xFFFF == 0 and t < self.easy_from and r.no_speech_prob[i] < 0.5:
                r.logprobs[i, :r.lens[i]] = -5.0
        return B.TranscribeResult(r.tokens, r.lens, r.logprobs, r.no_speech_prob, kw["eot"])

    def transcribe_windows(self, windows, rows, prompts, max_new, eot=-1, temperature=0.0, seed=0, no_speech_token=-1,
                           sot_index=0, sample_ids=None, budgets=None, prompt_len=None, sot_tail=None):
        assert not windows.closed and windows is self.sets[-1]
        self.n_decodes += 1
        if self.fail_at is not None and self.n_decodes == self.fail_at:
            raise RuntimeError("decode failed")
        windows.decodes.append((float(temperature), [int(r) for r in rows]))
        self.mel_calls -= 1
        return self.transcribe_mel(None, [windows.base[r] for r in rows], None, [windows.seek[r] for r in rows],
                                   [windows.n_frames[r] for r in rows], prompts, max_new, eot=eot, temperature=temperature,
                                   seed=seed, no_speech_token=no_speech_token, sample_ids=sample_ids)

    def align_windows(self, windows, rows, text_tokens, sot_seqs, no_timestamps, eot, medfilt_width=7, qk_scale=1.0):
        assert not windows.closed and windows is self.sets[-1]
        windows.aligns.append([int(r) for r in rows])
        return self.align_mel(None, [windows.base[r] for r in rows], None, [windows.seek[r] for r in rows],
                              [windows.n_frames[r] for r in rows], text_tokens, sot_seqs, no_timestamps, eot,
                              medfilt_width=medfilt_width, qk_scale=qk_scale, mem=B.WM_MEM_DEVICE)


RECS = [np.zeros(16000 * 70, np.float32), np.zeros(16000 * 50, np.float32), np.zeros(160, np.float32)]


def _run(vocab, reuse, words=True, **ctx_kw):
    ctx = FakeSetCtx(SCRIPT, **ctx_kw)
    kw = _fake_kw(language=[LANG_EN, LANG_ZH, LANG_EN], vocab=vocab, logprob_threshold=-1.0, reuse_encoder=reuse)
    if words:
        kw.update(word_timestamps=True, no_timestamps=NO_TS)
    return ctx, B.transcribe_long(ctx, RECS, **kw)


def test_one_encode_per_round_and_every_step_reads_its_todo_rows(vocab):
    ctx, out = _run(vocab, True)
    off_ctx, off = _run(vocab, False)
    assert out == off and not off_ctx.sets and off_ctx.mel_calls > 0
    assert ctx.mel_calls == 0                       # every decode of the run read a set
    n_rounds = max(len(o["windows"]) for o in out)
    assert len(ctx.sets) == n_rounds and all(s.closed == 1 for s in ctx.sets)
    seen = [0] * len(RECS)   # windows of each recording already met
    for s in ctx.sets:
        # the round's live recordings, in order, are the set's windows
        live = [r for r in range(len(RECS)) if seen[r] < len(out[r]["windows"])]
        wins = [out[r]["windows"][seen[r]] for r in live]
        assert s.seek == [w["seek"] for w in wins] and s.n_frames == [w["segment_size"] for w in wins]
        # fallback step k decodes the rows that took part in more than k steps: that step's todo
        n_steps = max(len(w["temperatures"]) for w in wins)
        assert len(s.decodes) == n_steps
        for k, (t, rows) in enumerate(s.decodes):
            assert rows == [i for i, w in enumerate(wins) if len(w["temperatures"]) > k]
            assert all(w["temperatures"][k] == t for i, w in enumerate(wins) if i in rows)
        # the word step: one align call, its rows the kept windows with text and at least 2 frames
        kept = [i for i, (r, w) in enumerate(zip(live, wins))
                if not w["skipped"] and any(t < EOT for t in w["tokens"]) and w["segment_size"] >= 2]
        assert s.aligns == ([kept] if kept else [])
        for r in live:
            seen[r] += 1
    # the hard recording did fall back, the others did not
    assert all(w["temperatures"] == [0.0, 0.2, 0.4] for w in out[0]["windows"] if not w["skipped"])
    assert all(w["temperatures"] == [0.0] for w in out[1]["windows"])


def test_without_words_no_align_call_reads_the_set(vocab):
    ctx, out = _run(vocab, True, words=False)
    assert out == _run(vocab, False, words=False)[1]
    assert ctx.sets and all(s.closed == 1 and not s.aligns for s in ctx.sets)


@pytest.mark.parametrize("fail_at", [1, 2, 5])
def test_the_set_is_freed_when_a_decode_raises(vocab, fail_at):
    ctx = FakeSetCtx(SCRIPT, fail_at=fail_at)
    with pytest.raises(RuntimeError):
        B.transcribe_long(ctx, RECS, **_fake_kw(language=[LANG_EN, LANG_ZH, LANG_EN], vocab=vocab, reuse_encoder=True))
    assert ctx.sets and all(s.closed == 1 for s in ctx.sets)


def test_default_makes_no_set(vocab):
    ctx = FakeSetCtx(SCRIPT)
    B.transcribe_long(ctx, RECS, **_fake_kw(language=[LANG_EN, LANG_ZH, LANG_EN], vocab=vocab))
    assert not ctx.sets and ctx.mel_calls > 0


# ---------------------------------------------------------------- the ctypes mirror against the header
_CTYPE = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "wm_mem": ctypes.c_int}


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "whisper_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"WM_API\s+(\w+)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        if "*" in a:
            args.append("pointer")
        else:
            args.append(_CTYPE[a.replace("const ", "").rsplit(" ", 1)[0]])
    return m.group(1), args


@pytest.mark.parametrize("name", ["wm_windows_encode", "wm_windows_count", "wm_transcribe_windows", "wm_transcribe_windows_beam",
                                  "wm_align_windows", "wm_windows_detect_language", "wm_windows_free", "wm_windows_bytes"])
def test_ctypes_signatures_match_the_header(pkg, name):
    lib = pkg.load_library()
    ret, want = _header_args(name)
    fn = getattr(lib, name)
    got = list(fn.argtypes)
    assert len(got) == len(want), (name, len(got), len(want))
    for g, w in zip(got, want):
        if w == "pointer":
            assert g is ctypes.c_void_p or issubclass(g, ctypes._Pointer), (name, g)
        else:
            assert g is w, (name, g, w)
    assert fn.restype is {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t}[ret]


def test_null_arguments_are_reported_without_a_device(pkg):
    lib = pkg.load_library()
    buf = np.zeros(8, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p(5)
    assert lib.wm_windows_encode(None, p, p, p, p, p, 1, 0, ctypes.byref(out)) == 1 and not out       # WM_ERR_INVALID
    assert b"null" in lib.wm_last_error()
    assert lib.wm_windows_encode(None, p, p, p, p, p, 1, 0, None) == 1
    assert lib.wm_transcribe_windows(None, None, None, 1, p, 3, None, 1, None, 1, float("nan"), 4, 5, None, p, p, None, None,
                                     None) == 1
    assert lib.wm_transcribe_windows_beam(None, None, None, 1, p, 3, None, 1, 2, 2, float("nan"), 4, 5, None, p, p, p, p, None,
                                          None, None) == 1
    assert lib.wm_align_windows(None, None, None, 1, p, 3, 1, 2, p, p, 1, 7, 1.0, p, p) == 1
    assert lib.wm_windows_detect_language(None, None, None, 1, 1, 2, 3, p, None) == 1
    assert b"null" in lib.wm_last_error()
    lib.wm_windows_free(None)
    assert lib.wm_windows_count(None) == -1 and lib.wm_windows_bytes(None) == 0
