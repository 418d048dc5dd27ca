"""wm_set_prompt_panel without a device: the plan (tx_plan.cpp wm_prompt_panel_plan, through the host-only hook) and the ragged
panel's attention plan against the restatements in tests/prompt_panel_ref.py; what Context.set_prompt_panel hands the C
function (on the stand-in library of tests/test_binding_calls_cpu.py); where transcribe_long(prompt_panel=...) puts its one
setter call (on the recording context of tests/test_longform_calls_cpu.py, against that file's committed golden logs); and
what the public header declares."""
import ctypes
import os
import re

import numpy as np
import pytest

import prompt_panel_ref as ref
import test_binding_calls_cpu as BC
import test_longform_calls_cpu as LC

B = BC.B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP = ctypes.POINTER(ctypes.c_int32)
PS = tuple(range(1, 41)) + (223, 224, 447)
LOG_CASES = ("defaults", "flat_prompt", "per_recording_prompts", "cond")   # MIN, STD, ragged (twice): whole logs in the golden


@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_prompt_panel_plan.argtypes = [ctypes.c_int] * 5 + [IP]
    lib.wmdbg_prompt_panel_plan.restype = ctypes.c_int
    lib.wmdbg_prompt_panel_plan_batch.argtypes = [ctypes.c_int, IP, IP]
    lib.wmdbg_prompt_panel_plan_batch.restype = ctypes.c_int
    lib.wmdbg_dec_attn_plan.argtypes = [IP, ctypes.c_int, IP]
    lib.wmdbg_dec_attn_plan.restype = ctypes.c_int
    lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.wmdbg_set_tuning(b"reset", 0)
    yield lib
    lib.wmdbg_set_tuning(b"reset", 0)


def _plan_cases(width):
    """every (G, P, sot_pos, acap on / off) at one width: G 1 .. 128, P of PS, sot_pos in [-1, P); an aligned group's first
    captured position is (P - 1) // 2 -- in front of, at and behind <|startoftranscript|> as sot_pos moves"""
    rows = []
    for P in PS:
        sot = np.arange(-1, P, dtype=np.int64)
        for acap in (-1, (P - 1) // 2):
            g, s = np.meshgrid(np.arange(1, 129, dtype=np.int64), sot, indexing="ij")
            n = g.size
            rows.append(np.stack([g.reshape(-1), np.full(n, width), np.full(n, P), s.reshape(-1), np.full(n, acap)], axis=1))
    return np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("width", range(1, 9))
def test_the_plan_is_its_restatement_and_covers_the_prompt_once(dbg, width):
    a = np.ascontiguousarray(_plan_cases(width))
    n = a.shape[0]
    assert n == 128 * 2 * sum(P + 1 for P in PS)
    out = np.full((n, 5), -1, dtype=np.int32)
    assert dbg.wmdbg_prompt_panel_plan_batch(n, a.ctypes.data_as(IP), out.ctypes.data_as(IP)) == 0
    G, _, P, sot, acap = (a[:, i].astype(np.int64) for i in range(5))
    want = ref.plan(G, width, P, sot, acap)
    for i, c in enumerate(ref.PLAN_COLS):
        bad = np.nonzero(out[:, i] != want[c])[0]
        assert bad.size == 0, "%s differs in %d cases, first %s: plan %d, restatement %d" % (c, bad.size, a[bad[0]].tolist(), out[bad[0], i], want[c][bad[0]])
    P0, C, w, sl, st = (out[:, i].astype(np.int64) for i in range(5))
    # P0 by the rule, spelled out once more
    assert (P0 == np.where(sot >= 0, np.where((acap >= 0) & (acap < sot), acap, sot), np.where(acap >= 0, np.minimum(acap, P - 1), P - 1))).all()
    on = w > 0
    assert (on == ((width > 1) & (P0 >= 2))).all()
    assert not out[~on, 1:].any()                      # width 1 or P0 < 2: no panel at all
    assert (C[on] * w[on] <= 128).all() and (w[on] <= width).all() and (C[on] >= 1).all()
    # the panels of a slice are [0, w), [w, 2 w), ...: the last one ends AT P0 (no panel reaches position P0) and none is empty
    assert ((st[on] - 1) * w[on] < P0[on]).all() and (st[on] * w[on] >= P0[on]).all()
    # the slices are [0, C), [C, 2 C), ...: every window in exactly one, none empty
    assert ((sl[on] - 1) * C[on] < G[on]).all() and (sl[on] * C[on] >= G[on]).all()
    if width == 8:   # three rows in one slice, a group that runs as slices, and one that fits a narrowed panel
        i = np.nonzero((G == 48) & (P == 19) & (sot == 16) & (acap == -1))[0][0]
        assert out[i].tolist() == [16, 16, 8, 3, 2]
        i = np.nonzero((G == 3) & (P == 20) & (sot == 17) & (acap == -1))[0][0]
        assert out[i].tolist() == [17, 3, 8, 1, 3]
        i = np.nonzero((G == 48) & (P == 20) & (sot == 17) & (acap == -1))[0][0]
        assert out[i].tolist() == [17, 24, 5, 2, 4]   # two slices of narrowed panels: 8 steps beat 3 x 3
        i = np.nonzero((G == 17) & (P == 20) & (sot == 17) & (acap == -1))[0][0]
        assert out[i].tolist() == [17, 17, 7, 1, 3]   # ONE narrowed panel


def test_the_scalar_hook_is_the_batch_hook_and_refuses_bad_arguments(dbg):
    out = np.zeros(5, dtype=np.int32)
    assert dbg.wmdbg_prompt_panel_plan(3, 8, 20, 17, -1, out.ctypes.data_as(IP)) == 0 and out.tolist() == [17, 3, 8, 1, 3]
    assert dbg.wmdbg_prompt_panel_plan(3, 8, 20, -1, -1, out.ctypes.data_as(IP)) == 0 and out.tolist() == [19, 3, 8, 1, 3]
    assert dbg.wmdbg_prompt_panel_plan(3, 8, 20, 17, 5, out.ctypes.data_as(IP)) == 0 and out.tolist() == [5, 3, 8, 1, 1]
    assert dbg.wmdbg_prompt_panel_plan(3, 1, 20, 17, -1, out.ctypes.data_as(IP)) == 0 and out.tolist() == [17, 0, 0, 0, 0]
    assert dbg.wmdbg_prompt_panel_plan(3, 8, 3, 0, -1, out.ctypes.data_as(IP)) == 0 and out.tolist() == [0, 0, 0, 0, 0]
    for bad in ((0, 8, 20, 17, -1), (129, 8, 20, 17, -1), (3, 0, 20, 17, -1), (3, 9, 20, 17, -1), (3, 8, 0, -1, -1), (3, 8, 20, 20, -1),
                (3, 8, 20, -2, -1), (3, 8, 20, 17, 20)):
        assert dbg.wmdbg_prompt_panel_plan(*bad, out.ctypes.data_as(IP)) == 1


def test_the_ragged_panel_attention_plan_is_its_restatement(dbg):
    """wm_plan_self_attention_panel with HAS_OFF over the panel test's (C, w) domain: the shape of the uniform panel, the
    ragged instantiation"""
    HAS_POS, HAS_OFF, HAS_PF = 1, 4, 8
    shapes = [(c, w) for w in range(1, 9) for c in range(1, 129) if c * w <= 128]
    T = 448
    done = 0
    for H, d in ((6, 384), (8, 512), (12, 768), (16, 1024), (20, 1280)):
        g = np.meshgrid(np.arange(len(shapes)), np.array([256, 128, 88, 80, 8]), np.array([0, 1]), np.array([0, 1]), indexing="ij")
        sh, cus, warm, off = (c.reshape(-1) for c in g)
        C, w = np.array([s[0] for s in shapes])[sh], np.array([s[1] for s in shapes])[sh]
        n = len(C)
        a = np.zeros((n, 16), dtype=np.int32)
        a[:, 0] = 4
        a[:, 2], a[:, 3], a[:, 4], a[:, 5] = C, w, H, T
        a[:, 9] = HAS_POS | warm * HAS_PF | off * HAS_OFF
        a[:, 10], a[:, 11], a[:, 12] = d, d, cus
        out = np.full((n, 16), -1, dtype=np.int32)
        assert dbg.wmdbg_dec_attn_plan(a.ctypes.data_as(IP), n, out.ctypes.data_as(IP)) == n
        want = ref.self_attention_panel_off(C, w, H, T, True, off == 1, warm == 1, d, d)
        for i, c in enumerate(ref.ATTN_COLS):
            got = out[:, i].astype(np.int64) & 0xffffffff
            exp = np.broadcast_to(want[c], (n,)).astype(np.int64) & 0xffffffff
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "H=%d: %s differs in %d cases, first at %d: plan %d, restatement %d" % (H, c, bad.size, bad[0], got[bad[0]], exp[bad[0]])
        assert not out[:, len(ref.ATTN_COLS):].any()
        assert set(out[off == 1, 1].tolist()) == {ref.SELF_OFF_PANEL} and set(out[off == 0, 1].tolist()) == {ref.SELF_PANEL}
        done += n
    assert done == 5 * len(shapes) * 5 * 2 * 2
    # refused like the uniform panel: too many rows, a width past the maximum, no device position
    bad = np.zeros((3, 16), dtype=np.int32)
    bad[:, 0] = 4
    bad[:, 2:6] = ((17, 8, 6, T), (1, 9, 6, T), (1, 8, 6, T))
    bad[:, 9] = (HAS_POS | HAS_OFF, HAS_POS | HAS_OFF, HAS_OFF)
    bad[:, 12] = 256
    out = np.full((3, 16), -1, dtype=np.int32)
    assert dbg.wmdbg_dec_attn_plan(bad.ctypes.data_as(IP), 3, out.ctypes.data_as(IP)) == 3
    assert out[:, 0].tolist() == [1, 1, 1] and not out[:, 1:14].any()


# ---------------------------------------------------------------- the binding ----
def test_set_prompt_panel_packs_one_int(monkeypatch):
    monkeypatch.setitem(BC.SPEC, "wm_set_prompt_panel", ("h width", {}, {}))
    ctx = BC.make_ctx()
    assert ctx.set_prompt_panel(8) is None
    assert ctx.set_prompt_panel(1) is None
    assert ctx.lib.calls == [["wm_set_prompt_panel", {"width": 8}], ["wm_set_prompt_panel", {"width": 1}]]
    assert ctx.lib.wm_set_prompt_panel.argtypes[1:] == [B.ctypes.c_int]


class PanelCtx(LC.RecCtx):
    def set_prompt_panel(self, *a, **kw):
        self._log("set_prompt_panel", a, kw)


def _run(case, **more):
    ctx = PanelCtx(case["script"], **case.get("ctx", {}))
    out = B.transcribe_long(ctx, [LC._rec(s) for s in LC.SECONDS], **dict(case["kw"], **more))
    return LC.json.loads(LC.json.dumps(LC.canon(dict(calls=ctx.calls, out=out))))


@pytest.mark.parametrize("name", LOG_CASES)
def test_prompt_panel_adds_exactly_one_setter_call_before_the_first_decode_call(name):
    case = LC.cases(None)[name]
    with open(LC.GOLDEN_FILE) as f:
        want = LC.json.load(f)["cases"][name]["full"]
    first = next(i for i, c in enumerate(want["calls"]) if c[0].startswith("transcribe_"))
    for width in (1, 8):
        got = _run(case, prompt_panel=width)
        assert got["calls"] == want["calls"][:first] + [["set_prompt_panel", [width], []]] + want["calls"][first:]
        assert got["out"] == want["out"]
    # the default, and None spelled out: the golden log
    assert _run(case) == want
    assert _run(case, prompt_panel=None) == want


def test_bad_widths_raise_before_any_call():
    case = LC.cases(None)["cond"]
    for bad in (0, 9, 2.5, True, -1, "8"):
        ctx = PanelCtx(case["script"])
        with pytest.raises(ValueError, match="prompt_panel"):
            B.transcribe_long(ctx, [LC._rec(s) for s in LC.SECONDS], **dict(case["kw"], prompt_panel=bad))
        assert ctx.calls == []


def test_the_header_declares_the_setter():
    with open(os.path.join(ROOT, "include", "whisper_mi355x.h")) as f:
        h = f.read()
    assert re.search(r"WM_API\s+int\s+wm_set_prompt_panel\s*\(\s*wm_ctx\s*\*\s*ctx\s*,\s*int\s+width\s*\)\s*;", h)
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("PROMPT PANELS"):h.index("wm_set_prompt_panel(wm_ctx")])   # the comment as one line
    for word in ("bit-identical for every width", "P0", "no_speech_prob", "wm_transcribe_mel_ragged", "wm_transcribe_windows_aligned",
                 "best-of", "beam-search", "wm_transcribe_mel_speculative", "WM_MAX_TEACHER_PANEL"):
        assert word in doc, word
    with open(os.path.join(ROOT, "include", "whisper_mi355x_debug.h")) as f:
        hd = f.read()
    for name in ("wmdbg_dec_self_attention_panel_off", "wmdbg_dec_embed_panel_off", "wmdbg_prompt_panel_plan", "wmdbg_last_prompt_prefill"):
        assert re.search(r"WM_API\s+int\s+%s\s*\(" % name, hd), name
