"""wm_set_teacher_panel without a device: what Context.set_teacher_panel hands the C function (on the stand-in library of
tests/test_binding_calls_cpu.py), where transcribe_long(teacher_panel=...) puts its one setter call (on the recording context
of tests/test_longform_calls_cpu.py, against that file's committed golden logs), and what the public header declares."""
import os
import re

import pytest

import test_binding_calls_cpu as BC
import test_longform_calls_cpu as LC

B = BC.B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD_CASES = ("words", "words_cond_hallucination")   # cases whose whole call log is in the golden


def test_set_teacher_panel_packs_one_int(monkeypatch):
    monkeypatch.setitem(BC.SPEC, "wm_set_teacher_panel", ("h width", {}, {}))
    ctx = BC.make_ctx()
    assert ctx.set_teacher_panel(8) is None
    assert ctx.set_teacher_panel(1) is None
    assert ctx.lib.calls == [["wm_set_teacher_panel", {"width": 8}], ["wm_set_teacher_panel", {"width": 1}]]
    assert ctx.lib.wm_set_teacher_panel.argtypes[1:] == [B.ctypes.c_int]


class PanelCtx(LC.RecCtx):
    def set_teacher_panel(self, *a, **kw):
        self._log("set_teacher_panel", a, kw)


def _run(case, **more):
    ctx = PanelCtx(case["script"], **case.get("ctx", {}))
    out = B.transcribe_long(ctx, [LC._rec(s) for s in LC.SECONDS], **dict(case["kw"], **more))
    return LC.json.loads(LC.json.dumps(LC.canon(dict(calls=ctx.calls, out=out))))


@pytest.mark.parametrize("name", WORD_CASES)
def test_teacher_panel_adds_exactly_one_setter_call_before_the_first_alignment(name, tmp_path):
    vocab = LC.make_vocab(tmp_path)
    try:
        case = LC.cases(vocab)[name]
        with open(LC.GOLDEN_FILE) as f:
            want = LC.json.load(f)["cases"][name]["full"]
        first = next(i for i, c in enumerate(want["calls"]) if c[0].startswith("align_"))
        got = _run(case, teacher_panel=8)
        assert got["calls"] == want["calls"][:first] + [["set_teacher_panel", [8], []]] + want["calls"][first:]
        assert got["out"] == want["out"]
        # the default, and None spelled out: the golden log
        assert _run(case) == want
        assert _run(case, teacher_panel=None) == want
    finally:
        vocab.close()


def test_teacher_panel_without_words_makes_no_call_and_bad_widths_raise_before_any_call():
    case = LC.cases(None)["defaults"]
    with open(LC.GOLDEN_FILE) as f:
        want = LC.json.load(f)["cases"]["defaults"]["full"]
    assert _run(case, teacher_panel=4) == want
    for bad in (0, 9, -1, 2.5, True):
        ctx = PanelCtx(case["script"])
        with pytest.raises(ValueError, match="teacher_panel"):
            B.transcribe_long(ctx, [LC._rec(s) for s in LC.SECONDS], **dict(case["kw"], teacher_panel=bad))
        assert ctx.calls == []


def test_the_header_declares_the_setter_and_ties_the_width_to_best_of():
    with open(os.path.join(ROOT, "include", "whisper_mi355x.h")) as f:
        h = f.read()
    assert re.search(r"WM_API\s+int\s+wm_set_teacher_panel\s*\(\s*wm_ctx\s*\*\s*ctx\s*,\s*int\s+width\s*\)\s*;", h)
    width = int(re.search(r"#define\s+WM_MAX_TEACHER_PANEL\s+(\d+)", h).group(1))
    best_of = int(re.search(r"#define\s+WM_MAX_BEST_OF\s+(\d+)", h).group(1))
    assert width == best_of == 8 == B.MAX_TEACHER_PANEL
    assert "bit-identical for every width" in h
