"""Characterization of the Context call wrappers without a device: a Context made by object.__new__ over a stand-in `lib`
whose functions record what they are handed, compared with tests/golden/binding_calls_parent.json.

What is recorded of a C call: scalars as given (NaN as "nan"); an input pointer as the array it points to, READ BACK FROM
THE ADDRESS with the dtype of the C signature and the shape the call's own scalar arguments imply; None as None; an output
pointer as that dtype and shape only (the stand-in then fills it, so that the wrapper has a result to pack); a device
pointer as its value; wm_decode_opts by its fields.  And of the wrapper: what it returned.

The golden is this project's own recorded result: `python tests/test_binding_calls_cpu.py --record <commit>` run at the
commit BEFORE the wrappers' packing was factored (the commit is named inside the file); not to be recorded from later code."""
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

B = importlib.import_module("openai_whisper_coreml_amd.binding")
GOLDEN_FILE = os.path.join(GOLDEN, "binding_calls_parent.json")
I32, I64, F32, U32 = "int32", "int64", "float32", "uint32"
SET_HANDLE, DEVICE_MEL = 0x5E70, 0xD000

# name -> (argument names, {input pointer: (dtype, shape)}, {output pointer: (dtype, shape)}); shapes are expressions over the
# call's scalars.  `blob` is the one host input whose extent no scalar states (the mel, the pcm): the test says it.
_WIN = dict(base=(I64, "B"), mel_len=(I32, "B"), seek=(I32, "B"), n_frames=(I32, "B"))
_PROMPT = dict(prompts=(I32, "B, stride"), prompt_len=(I32, "B"), ids=(U32, "B"))
_ALIGN_IN = dict(sot=(I32, "B, n_sot"), tt=(I32, "B, max(max_text, 1)"), nt=(I32, "B"))
_ALIGN_OUT = dict(start=(I32, "B, max_text + 1"), probs=(F32, "B, max_text"))
_ONE = dict(toks=(I32, "B, max_new"), lens=(I32, "B"), lp=(F32, "B, max_new"), ns=(F32, "B"))
_CAND = dict(toks=(I32, "B, max(N, 1), max_new"), lens=(I32, "B, max(N, 1)"), lp=(F32, "B, max(N, 1), max_new"), ns=(F32, "B"),
             best=(I32, "B"))
_BEAM = dict(toks=(I32, "B, max(N, C, 1), max_new"), lens=(I32, "B, max(N, C, 1)"), n_hyp=(I32, "B"),
             sums=(F32, "B, max(N, C, 1)"), lp=(F32, "B, max(N, C, 1), max_new"), ns=(F32, "B"), best=(I32, "B"))
SPEC = {
    "wm_set_token_budgets": ("h budgets n", dict(budgets=(I32, "n")), {}),
    "wm_transcribe_mel": ("h blob base mel_len seek n_frames B prompts stride ids max_new eot opts toks lens lp ns mem",
                          dict(_WIN, **_PROMPT), _ONE),
    "wm_transcribe_mel_ragged": ("h blob base mel_len seek n_frames B prompts stride prompt_len sot_tail ids max_new eot opts "
                                 "toks lens lp ns mem", dict(_WIN, **_PROMPT), _ONE),
    "wm_transcribe_mel_best_of": ("h blob base mel_len seek n_frames B prompts stride prompt_len sot_tail ids N length_penalty "
                                  "max_new eot opts toks lens lp ns best mem", dict(_WIN, **_PROMPT), _CAND),
    "wm_transcribe_mel_beam": ("h blob base mel_len seek n_frames B prompts stride prompt_len sot_tail N C length_penalty max_new "
                               "eot opts toks lens n_hyp sums lp ns best mem", dict(_WIN, **_PROMPT), _BEAM),
    "wm_windows_encode": ("h blob base mel_len seek n_frames B mem out_handle", _WIN, {}),
    "wm_transcribe_windows": ("h set rows B prompts stride prompt_len sot_tail ids N length_penalty max_new eot opts toks lens lp "
                              "ns best", dict(_PROMPT, rows=(I32, "B")), _CAND),
    "wm_transcribe_windows_beam": ("h set rows B prompts stride prompt_len sot_tail N C length_penalty max_new eot opts toks lens "
                                   "n_hyp sums lp ns best", dict(_PROMPT, rows=(I32, "B")), _BEAM),
    "wm_align": ("h blob dtype B sot n_sot no_timestamps eot tt nt max_text n_frames medfilt_width qk_scale start probs mem",
                 dict(_ALIGN_IN, sot=(I32, "n_sot"), n_frames=(I32, "B")), _ALIGN_OUT),
    "wm_align_mel": ("h blob base mel_len seek n_frames B sot n_sot no_timestamps eot tt nt max_text medfilt_width qk_scale start "
                     "probs mem", dict(_WIN, **_ALIGN_IN), _ALIGN_OUT),
    "wm_align_windows": ("h set rows B sot n_sot no_timestamps eot tt nt max_text medfilt_width qk_scale start probs",
                         dict(_ALIGN_IN, rows=(I32, "B")), _ALIGN_OUT),
    "wmdbg_align_capture": ("h matrix", {}, {}),
}
FILL = dict(lens=1, lp=-0.5, ns=0.25, n_hyp=1, sums=-1.5, probs=0.5)


def _at(address, dtype, shape):
    n = int(np.prod(shape, dtype=np.int64))
    if n == 0:
        return np.zeros(shape, dtype=dtype)
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(address)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return dict(dtype=str(x.dtype), shape=list(x.shape), c_contiguous=bool(x.flags["C_CONTIGUOUS"]),
                    values=plain(x.reshape(-1).tolist()))
    if isinstance(x, np.generic):
        x = x.item()
    if isinstance(x, float) and x != x:
        return "nan"
    if isinstance(x, float) and x in (float("inf"), float("-inf")):
        return str(x)
    return x


class FakeLib:
    """lib.<name>(...) records the call by SPEC and returns WM_OK; wmdbg_* exist with debug=True only."""

    def __init__(self, debug=False):
        self.calls, self.blob, self.n_windows, self.debug = [], None, 0, debug

    def wm_last_error(self):
        return b"stand-in"

    def wm_destroy(self, h):
        pass

    def wm_windows_free(self, h):
        pass

    def wm_windows_count(self, h):
        return self.n_windows

    def __getattr__(self, name):
        if name not in SPEC or (name.startswith("wmdbg_") and not self.__dict__.get("debug")):
            raise AttributeError(name)

        def fn(*args):
            return self._record(name, args)
        self.__dict__[name] = fn    # (the wrappers set argtypes / restype on it)
        return fn

    def _record(self, name, args):
        names, ins, outs = SPEC[name]
        names = names.split()
        assert len(names) == len(args), (name, len(args))
        d = dict(zip(names, args))
        scal = {k: v for k, v in d.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
        rec = {}
        for k, v in d.items():
            if k == "h":
                continue
            if v is None or k in scal:
                rec[k] = plain(v)
            elif k == "opts":
                o = v._obj
                rec[k] = dict(temperature=plain(float(o.temperature)), seed=int(o.seed), no_speech_token=int(o.no_speech_token),
                              sot_index=int(o.sot_index))
            elif k == "out_handle":
                v._obj.value = SET_HANDLE
                rec[k] = "handle"
            elif k == "set":
                rec[k] = "set:%x" % v.value
            elif k == "matrix":
                rec[k] = "matrix"
            elif k == "blob":
                if d.get("mem", B.WM_MEM_HOST) == B.WM_MEM_DEVICE:
                    rec[k] = "device:%x" % v.value
                else:
                    rec[k] = plain(_at(v.value, *self.blob))
            elif k in ins:
                rec[k] = plain(_at(v.value, ins[k][0], eval("(%s,)" % ins[k][1], {}, scal)))
            else:
                dtype, shape = outs[k][0], eval("(%s,)" % outs[k][1], {}, scal)
                rec[k] = dict(dtype=dtype, shape=list(shape))
                out = _at(v.value, dtype, shape)
                if k == "toks":
                    out[...] = d["eot"]
                elif k == "best":
                    out[...] = np.arange(shape[0]) % eval("(%s,)" % outs["toks"][1], {}, scal)[1]
                elif k == "start":
                    out[...] = np.arange(out.size).reshape(shape)
                else:
                    out[...] = FILL[k]
        self.calls.append([name, rec])
        return B.WM_OK


def make_ctx(debug=False):
    ctx = object.__new__(B.Context)
    ctx.lib, ctx.handle = FakeLib(debug), ctypes.c_void_p(0xC0DE)
    ctx.dims = dict(n_mels=80, n_text_ctx=64, n_vocab=128)
    return ctx


def result(r):
    """what a wrapper returned"""
    if isinstance(r, B.Windows):
        return dict(windows=plain(r.n_frames), handle=r.handle.value)
    if isinstance(r, tuple):   # (the captured matrix, uninitialised here, by dtype and shape)
        return [dict(dtype=str(x.dtype), shape=list(x.shape)) if isinstance(x, np.ndarray) and x.size > 4096 else plain(x)
                for x in r]
    d = {k: plain(v) for k, v in vars(r).items() if k != "selected"}
    d["type"] = type(r).__name__
    if hasattr(r, "selected"):
        d["selected"] = result(r.selected)
    return d


MEL = np.arange(48, dtype=np.float32) / 8
PCM = (np.arange(24, dtype=np.int16) - 5).reshape(3, 8)
DEV = ctypes.c_void_p(DEVICE_MEL)
BASE3, LEN3, SEEK3, NF3 = [0, 16, 32], [11, 12, 13], [0, 3, 5], [7, 6, 2]
P3 = [[9, 1, 2, 3], [9, 1, 2, 3], [9, 4, 5, 6]]
RAGGED = [[1, 2, 3], [8, 7, 1, 2, 3], [9, 1, 2, 4]]
TEXT = [[5, 6, 7], [], [8]]
SOT3 = [[1, 2, 3], [1, 4, 3], [1, 5, 3]]
HOST, DEVICE = B.WM_MEM_HOST, B.WM_MEM_DEVICE


def _set(ctx, n=3):
    ctx.lib.n_windows = n
    return B.Windows(ctx, ctypes.c_void_p(SET_HANDLE), np.arange(n, dtype=np.int32) + 2)


def _opts(t=0.25, seed=77, ns=47, sot=1):
    return B.wm_decode_opts(t, seed, ns, sot)


CASES = {
    # transcribe_mel_raw: uniform table, ragged lists, prompt_len, sot_tail on a uniform table, broadcast scalars, device mel
    "mel_raw_uniform": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, SEEK3, NF3, np.array(P3), 4, 50, _opts(), [3, 2, 1 << 31]),
    "mel_raw_one_prompt_scalars_device": lambda c: c.transcribe_mel_raw(DEV, BASE3, 16, 0, 3000, [9, 1, 2], 5, 50, None, None,
                                                                        logprobs=False, no_speech=True, mem=DEVICE),
    "mel_raw_ragged_lists": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, SEEK3, NF3, RAGGED, 4, 50, _opts(), [1, 2, 3],
                                                           sot_tail=3, budgets=[4, 3, 2]),
    "mel_raw_ragged_default_tail": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, SEEK3, NF3, RAGGED, 4, 50, _opts()),
    "mel_raw_prompt_len": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, 2, NF3, np.array(P3), 4, 50, _opts(),
                                                         prompt_len=[4, 2, 3], sot_tail=2),
    "mel_raw_sot_tail_uniform": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, 50, _opts(), sot_tail=3),
    "mel_raw_sot_tail_without_opts": lambda c: c.transcribe_mel_raw(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, 50, None, sot_tail=3),
    # transcribe_mel: the three entries
    "mel_plain": lambda c: c.transcribe_mel(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, eot=50, temperature=0.5, seed=-1,
                                            no_speech_token=47, sot_index=1, sample_ids=[5, 6, 7]),
    "mel_plain_no_speech_off": lambda c: c.transcribe_mel(DEV, BASE3[:2], LEN3[:2], SEEK3[:2], NF3[:2], RAGGED[:2], 4, eot=50,
                                                          sot_tail=3, mem=DEVICE),
    "mel_best_of_entry": lambda c: c.transcribe_mel(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, eot=50, temperature=0.5, seed=3,
                                                    no_speech_token=47, sot_index=1, sample_ids=[5, 6, 7], best_of=3,
                                                    length_penalty=0.5, budgets=[1, 2, 3]),
    "mel_beam_entry": lambda c: c.transcribe_mel(MEL, BASE3, LEN3, SEEK3, NF3, RAGGED, 4, eot=50, no_speech_token=47, sot_tail=3,
                                                 sample_ids=[5, 6, 7], beam_size=2, patience=1.5),
    "mel_best_of": lambda c: c.transcribe_mel_best_of(MEL, BASE3, LEN3, 1, 9, P3, 4, 2, eot=50, temperature=0.75, seed=1 << 70,
                                                      no_speech_token=47, sot_index=1, sample_ids=[5, 6, 7]),
    "mel_best_of_ragged_device": lambda c: c.transcribe_mel_best_of(DEV, BASE3, LEN3, SEEK3, NF3, RAGGED, 4, 3, eot=50,
                                                                    temperature=1.0, sot_tail=3, mem=DEVICE, length_penalty=1.0),
    "mel_best_of_zero": lambda c: c.transcribe_mel_best_of(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, 0, eot=50),
    "mel_beam_patience": lambda c: c.transcribe_mel_beam(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, 2, eot=50, patience=2.5,
                                                         no_speech_token=47, sot_index=1, length_penalty=0.25),
    "mel_beam_max_candidates": lambda c: c.transcribe_mel_beam(DEV, BASE3, LEN3, SEEK3, 3000, RAGGED, 4, 3, eot=50,
                                                               max_candidates=2, sot_tail=3, mem=DEVICE, budgets=[1, 1, 1]),
    "mel_beam_default": lambda c: c.transcribe_mel_beam(MEL, BASE3, LEN3, SEEK3, NF3, P3, 4, 3, eot=50, prompt_len=[4, 3, 2]),
    # window sets
    "encode_windows_host": lambda c: c.encode_windows(MEL, BASE3, LEN3, SEEK3, NF3),
    "encode_windows_device_scalars": lambda c: c.encode_windows(DEV, np.array(BASE3)[[0, 2]], 16, 0, 3000, mem=DEVICE),
    "windows_plain": lambda c: c.transcribe_windows(_set(c), [2, 0], np.array(P3)[[2, 0]], 4, eot=50, temperature=0.5, seed=9,
                                                    no_speech_token=47, sot_index=1, sample_ids=[8, 9]),
    "windows_all_rows_ragged": lambda c: c.transcribe_windows(_set(c), None, RAGGED, 4, eot=50, sot_tail=3, budgets=[2, 2, 2]),
    "windows_best_of_entry": lambda c: c.transcribe_windows(_set(c), [1], [P3[1]], 4, eot=50, temperature=0.25, seed=2,
                                                            no_speech_token=47, sot_index=1, sample_ids=[4], best_of=2,
                                                            length_penalty=2.0),
    "windows_beam_entry": lambda c: c.transcribe_windows(_set(c), [0, 1, 2], RAGGED, 4, eot=50, no_speech_token=47, sot_tail=3,
                                                         sample_ids=[1, 2, 3], beam_size=3, patience=1.0, length_penalty=0.5),
    "windows_best_of": lambda c: c.transcribe_windows_best_of(_set(c), [0, 2], [P3[0], P3[2]], 4, 3, eot=50, temperature=0.5, seed=5,
                                                              no_speech_token=47, sot_index=1, sample_ids=[1, 2]),
    "windows_best_of_default_n": lambda c: c.transcribe_windows_best_of(_set(c), None, P3[0], 4, eot=50, prompt_len=[4, 4, 1]),
    "windows_beam_all_rows": lambda c: c.transcribe_windows_beam(_set(c), None, P3, 4, 2, eot=50, patience=1.5, no_speech_token=47,
                                                                 sot_index=1),
    "windows_beam_rows_repeated": lambda c: c.transcribe_windows_beam(_set(c), [1, 1, 0, 1], [RAGGED[1], RAGGED[1], RAGGED[0],
                                                                      RAGGED[2]], 4, 2, eot=50, max_candidates=5, sot_tail=3,
                                                                      length_penalty=1.0, budgets=[3, 3, 3, 3]),
    # alignment
    "align": lambda c: c.align(PCM, TEXT, [1, 2, 3], 48, 50),
    "align_n_frames_scalar": lambda c: c.align(PCM.astype(np.float32), np.array([[5, 6], [7, 8], [9, 10]]), [1, 2, 3], 48, 50,
                                               n_frames=1000, medfilt_width=5, qk_scale=0.5),
    "align_n_frames_array_no_text": lambda c: c.align(PCM, [[], [], []], [1, 2], 48, 50, n_frames=[10, 20, 30]),
    "align_capture": lambda c: c.align(PCM, TEXT, [1, 2, 3], 48, 50, capture_matrix=True),
    "align_mel_one_sot": lambda c: c.align_mel(MEL, BASE3, LEN3, SEEK3, NF3, TEXT, [1, 2, 3], 48, 50),
    "align_mel_per_row_sot_device_scalars": lambda c: c.align_mel(DEV, BASE3, 16, 0, 3000, TEXT, SOT3, 48, 50, medfilt_width=3,
                                                                  qk_scale=2.0, mem=DEVICE),
    "align_mel_capture": lambda c: c.align_mel(MEL, BASE3, LEN3, SEEK3, NF3, TEXT, SOT3, 48, 50, capture_matrix=True),
    "align_windows_one_sot": lambda c: c.align_windows(_set(c), [2, 0], [TEXT[2], TEXT[0]], [1, 2, 3], 48, 50),
    "align_windows_per_row_sot": lambda c: c.align_windows(_set(c), None, TEXT, SOT3, 48, 50, medfilt_width=9, qk_scale=0.25),
}
DEBUG_CASES = ("align_capture", "align_mel_capture")
BLOBS = {"align": ("int16", (3, 8)), "align_n_frames_scalar": ("float32", (3, 8)), "align_n_frames_array_no_text": ("int16", (3, 8)),
         "align_capture": ("int16", (3, 8))}


def run_case(name):
    ctx = make_ctx(debug=name in DEBUG_CASES)
    ctx.lib.blob = BLOBS.get(name, ("float32", (MEL.size,)))
    r = CASES[name](ctx)
    got = dict(calls=ctx.lib.calls, result=result(r))
    if isinstance(r, B.Windows):
        r.close()
    return json.loads(json.dumps(got))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_golden_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_c_calls_and_results_are_the_parents(golden, name):
    got = run_case(name)
    want = golden["cases"][name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got["result"] == want["result"]


def test_length_penalty_none_is_nan_and_windows_without_best_of_is_candidate_0(golden):
    """two things the golden must hold, read from it"""
    c = golden["cases"]
    assert c["mel_best_of"]["calls"][-1][1]["length_penalty"] == "nan"
    assert c["windows_beam_all_rows"]["calls"][-1][1]["length_penalty"] == "nan"
    plain_call = c["windows_plain"]["calls"][-1]
    assert plain_call[0] == "wm_transcribe_windows" and plain_call[1]["N"] == 1
    assert c["windows_plain"]["result"]["type"] == "TranscribeResult" and "candidate" not in c["windows_plain"]["result"]
    assert c["windows_all_rows_ragged"]["calls"][-1][1]["rows"] is None


def test_value_errors_keep_their_messages():
    mel = (MEL, BASE3, LEN3, SEEK3, NF3)
    for call, text in (
            (lambda c: c.transcribe_mel_raw(*mel, np.array(P3), 4, 50, _opts(), prompt_len=[4, 2]), "prompt_len: one length per row"),
            (lambda c: c.transcribe_windows_best_of(_set(c), [0], RAGGED, 4, eot=50), "prompt_len: one length per row"),
            (lambda c: c.transcribe_mel_beam(*mel, P3, 4, 2, patience=1.0, max_candidates=2), "give patience or max_candidates, not both"),
            (lambda c: c.transcribe_windows_beam(_set(c), None, P3, 4, 2, patience=1.0, max_candidates=2),
             "give patience or max_candidates, not both"),
            (lambda c: c.transcribe_mel_beam(*mel, P3, 4, 9), "beam_size must be an integer in 1 .. 8"),
            (lambda c: c.transcribe_windows_beam(_set(c), None, P3, 4, 2, patience=0.0), "patience must be positive"),
            (lambda c: c.transcribe_windows_beam(_set(c), None, P3, 4, 8, patience=3.0),
             "round(beam_size * patience) = 24 outside 1 .. 16"),
            (lambda c: c.transcribe_mel(*mel, P3, 4, beam_size=2, best_of=2), "beam_size and best_of exclude each other (openai-whisper)"),
            (lambda c: c.transcribe_windows(_set(c), None, P3, 4, patience=1.0, best_of=2),
             "beam_size and best_of exclude each other (openai-whisper)"),
            (lambda c: c.transcribe_mel(*mel, P3, 4, beam_size=2, temperature=0.5), "beam search decodes at temperature 0"),
            (lambda c: c.transcribe_windows(_set(c), None, P3, 4, beam_size=2, temperature=0.5), "beam search decodes at temperature 0"),
            (lambda c: c.transcribe_mel(*mel, P3, 4, patience=2.0), "patience requires beam_size to be given"),
            (lambda c: c.transcribe_windows(_set(c), None, P3, 4, patience=2.0), "patience requires beam_size to be given"),
            (lambda c: c.align(PCM, TEXT[:2], [1, 2, 3], 48, 50), "text_tokens: 2 lists for 3 chunks"),
            (lambda c: c.align_mel(*mel, TEXT[:2], [1, 2, 3], 48, 50), "text_tokens: 2 lists for 3 windows"),
            (lambda c: c.align_windows(_set(c), [0, 1], TEXT, [1, 2, 3], 48, 50), "text_tokens: 3 lists for 2 windows"),
            (lambda c: c.align_mel(*mel, TEXT, SOT3[:2], 48, 50), "sot_seqs: one start sequence, or one per window"),
            (lambda c: c.align_windows(_set(c), None, TEXT, [SOT3], 48, 50), "sot_seqs: one start sequence, or one per window")):
        ctx = make_ctx()
        with pytest.raises(ValueError) as e:
            call(ctx)
        assert str(e.value) == text
        assert [c[0] for c in ctx.lib.calls if c[0] != "wm_set_token_budgets"] == []
    for call in (lambda c: c.align(PCM, TEXT, [1, 2, 3], 48, 50, capture_matrix=True),
                 lambda c: c.align_mel(*mel, TEXT, SOT3, 48, 50, capture_matrix=True)):
        ctx = make_ctx()
        with pytest.raises(B.WhisperError) as e:
            call(ctx)
        assert str(e.value) == "wm status -1: capture_matrix needs the debug library: Context(dims, debug=True)"
        assert ctx.lib.calls == []


def record(commit):
    """Write the golden from the code as it stands: for the parent commit only (see the module's docstring)."""
    out = dict(recorded_at=commit, cases={name: run_case(name) for name in sorted(CASES)})
    with open(GOLDEN_FILE, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d bytes" % (GOLDEN_FILE, len(out["cases"]), os.path.getsize(GOLDEN_FILE)))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        raise SystemExit("usage: python tests/test_binding_calls_cpu.py --record <commit the golden is recorded at>")
    record(sys.argv[2])
