"""The argument checks of the eight transcribe entry points (csrc/transcribe.cpp), through the raw C ABI on a tiny synthetic
model (tiny.en geometry): one invalid call per check, plus the calls where two checks apply at once and their order decides
which error comes back.  Every (status, wm_last_error()) pair is compared with tests/golden/transcribe_errors_parent.json,
recorded from the commit before the call was restated as one request value (TxCall) -- the file is that commit's own output
and is not re-recorded.  A call that fails its checks still consumes the token budgets set for it: budgets of one token per
row are set before every failing call on the model's context, and a valid two-row call right after it, made with no budgets
set, must come back with the full max_new."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "transcribe_errors_parent.json")
SOT, NO_TS, EOT, NS_TOK = 50257, 50362, 50256, 50361
NEW = 3
MEL = ("mel", "mel_base", "mel_len", "seek", "n_frames")
TAIL = ("max_new", "eot", "opts", "tokens_out", "lens_out", "logprobs_out", "no_speech_out")
RAGGED = ("B", "prompts", "prompt_stride", "prompt_len", "sot_tail")
# the parameters of each entry point in the order of include/whisper_mi355x.h
ENTRIES = {
    "wm_transcribe_greedy": ("ctx", "pcm", "pcm_dtype", "B", "prompts", "n_prompt", "max_new", "eot", "tokens_out", "lens_out", "mem"),
    "wm_transcribe": ("ctx", "pcm", "pcm_dtype", "B", "prompts", "n_prompt") + TAIL + ("mem",),
    "wm_transcribe_mel": ("ctx",) + MEL + ("B", "prompts", "n_prompt", "sample_ids") + TAIL + ("mem",),
    "wm_transcribe_mel_ragged": ("ctx",) + MEL + RAGGED + ("sample_ids",) + TAIL + ("mem",),
    "wm_transcribe_mel_best_of": ("ctx",) + MEL + RAGGED + ("sample_ids", "best_of", "length_penalty") + TAIL + ("best_out", "mem"),
    "wm_transcribe_windows": ("ctx", "set", "rows") + RAGGED + ("sample_ids", "best_of", "length_penalty") + TAIL + ("best_out",),
    "wm_transcribe_mel_beam": ("ctx",) + MEL + RAGGED + ("beam_size", "max_candidates", "length_penalty") + TAIL[:5]
                              + ("n_hyp_out", "sums_out", "logprobs_out", "no_speech_out", "best_out", "mem"),
    "wm_transcribe_windows_beam": ("ctx", "set", "rows") + RAGGED + ("beam_size", "max_candidates", "length_penalty") + TAIL[:5]
                                  + ("n_hyp_out", "sums_out", "logprobs_out", "no_speech_out", "best_out"),
}
SHORT = {"greedy": "wm_transcribe_greedy", "plain": "wm_transcribe", "mel": "wm_transcribe_mel", "ragged": "wm_transcribe_mel_ragged",
         "best_of": "wm_transcribe_mel_best_of", "windows": "wm_transcribe_windows", "beam": "wm_transcribe_mel_beam",
         "windows_beam": "wm_transcribe_windows_beam"}


def _i32(*v):
    return np.array(v, dtype=np.int32)


class Env:
    """The contexts, the two windows and the valid value of every parameter (B = 2)."""

    def __init__(self, b):
        self.b, self.lib = b, b.load_debug_library()
        dims = dict(b.MODEL_DIMS["tiny.en"])
        self.V = dims["n_vocab"]
        self.ctx = b.Context(dims, debug=True)
        self.ctx.init_synthetic(23, matrix_gain=4.0)
        self.ctx.finalize()
        self.other = b.Context(dims, debug=True)       # the same model in another context: its sets are not ours
        self.other.init_synthetic(23, matrix_gain=4.0)
        self.other.finalize()
        self.unfinal = b.Context(dims, debug=True)     # weights never finalised
        self.frontend = b.Context(debug=True)                  # no model at all
        rng = np.random.default_rng(5)
        mel = (0.5 * rng.standard_normal((80, 3000))).astype(np.float32)   # one block, both rows read it
        w = (mel, _i32(0, 0).astype(np.int64), 3000, _i32(0, 100), _i32(3000, 1500))
        self.set = self.ctx.encode_windows(*w)
        self.other_set = self.other.encode_windows(*w)
        self.opts = b.wm_decode_opts(0.0, 7, -1, 0)
        self.keep = []
        self.valid = dict(
            ctx=self.ctx.handle, pcm=np.zeros((2, 480000), dtype=np.float32), pcm_dtype=b.WM_F32, B=2, mem=b.WM_MEM_HOST,
            mel=mel, mel_base=w[1], mel_len=_i32(3000, 3000), seek=w[3], n_frames=w[4], set=self.set.handle, rows=None,
            prompts=_i32(SOT, NO_TS, SOT, NO_TS), n_prompt=2, prompt_stride=2, prompt_len=None, sot_tail=1, sample_ids=None,
            best_of=2, beam_size=2, max_candidates=2, length_penalty=float("nan"), max_new=NEW, eot=-1, opts=None,
            tokens_out=np.zeros(2 * 16 * NEW, dtype=np.int32), lens_out=np.zeros(2 * 16, dtype=np.int32),
            logprobs_out=None, no_speech_out=None, best_out=None, n_hyp_out=np.zeros(2, dtype=np.int32),
            sums_out=np.zeros(2 * 16, dtype=np.float32))

    def raw(self, v):
        if v is None or isinstance(v, (int, float)):
            return v
        if isinstance(v, np.ndarray):
            self.keep.append(v)
            return v.ctypes.data
        if isinstance(v, ctypes.Structure):
            self.keep.append(v)
            return ctypes.addressof(v)
        return v   # a handle

    def call(self, entry, **over):
        """(status, message) of one call of the entry point with the valid arguments, `over` replacing some"""
        a = dict(self.valid, **over)
        st = getattr(self.lib, SHORT[entry])(*[self.raw(a[p]) for p in ENTRIES[SHORT[entry]]])
        return [int(st), self.lib.wm_last_error().decode("utf-8", "replace") if st else ""]

    def follow_up(self):
        """a valid two-row call with no budgets set: the rows' lens"""
        st, msg = self.call("mel")
        return self.valid["lens_out"][:2].tolist() if st == 0 else msg

    def tuning(self, key, value):
        self.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
        assert self.lib.wmdbg_set_tuning(key, value) == 0

    def close(self):
        self.set.close()
        self.other_set.close()
        for c in (self.ctx, self.other, self.unfinal, self.frontend):
            c.close()


def _opts(b, T=0.0, ns=-1, sot=0):
    return b.wm_decode_opts(T, 7, ns, sot)


def cases(e):
    """(name, entry, overrides, budgets set before the call or None, setup or None): one per check, then the orders"""
    b, V = e.b, e.V
    ns_out = np.zeros(2, dtype=np.float32)
    rag = dict(prompts=_i32(SOT, NO_TS, 5, SOT, NO_TS, 0), prompt_stride=3, prompt_len=_i32(3, 2))
    f32 = (lambda: e.ctx.set_precision(True), lambda: e.ctx.set_precision(False))
    rep_f32 = (lambda: (e.ctx.set_repetition_rules(1.5, 0, EOT), e.ctx.set_precision(True)),
               lambda: (e.ctx.set_precision(False), e.ctx.set_repetition_rules()))
    solo = (lambda: e.tuning(b"lane_solo_cus", 32), lambda: e.tuning(b"reset", 0))
    one = [1, 1]
    out = [
        # ---- the entry points' own null-pointer checks
        ("mel_null_mel", "mel", dict(mel=None), one, None),
        ("mel_null_seek", "mel", dict(seek=None), one, None),
        ("ragged_null_n_frames", "ragged", dict(rag, n_frames=None), one, None),
        ("ragged_null_prompt_len", "ragged", dict(rag, prompt_len=None), one, None),
        ("ragged_stride_0", "ragged", dict(rag, prompt_stride=0), one, None),
        # ---- best-of
        ("best_of_null_mel_base", "best_of", dict(mel_base=None), one, None),
        ("windows_null_set", "windows", dict(set=None), one, None),
        ("best_of_stride_0", "best_of", dict(prompt_stride=0), one, None),
        ("windows_stride_negative", "windows", dict(prompt_stride=-3), one, None),
        ("best_of_0", "best_of", dict(best_of=0), one, None),
        ("windows_best_of_9", "windows", dict(best_of=9), one, None),
        ("best_of_length_penalty", "best_of", dict(length_penalty=1.5), one, None),
        ("best_of_B_0", "best_of", dict(B=0), one, None),
        ("windows_max_new_0", "windows", dict(max_new=0), one, None),
        # ---- beam
        ("beam_null_mel_len", "beam", dict(mel_len=None), one, None),
        ("windows_beam_null_set", "windows_beam", dict(set=None), one, None),
        ("beam_null_n_hyp", "beam", dict(n_hyp_out=None), one, None),
        ("windows_beam_null_sums", "windows_beam", dict(sums_out=None), one, None),
        ("beam_stride_0", "beam", dict(prompt_stride=0), one, None),
        ("beam_size_0", "beam", dict(beam_size=0), one, None),
        ("windows_beam_size_9", "windows_beam", dict(beam_size=9), one, None),
        ("beam_max_candidates_0", "beam", dict(max_candidates=0), one, None),
        ("beam_max_candidates_17", "beam", dict(max_candidates=17), one, None),
        ("beam_length_penalty", "beam", dict(length_penalty=-0.25), one, None),
        ("beam_B_0", "beam", dict(B=0), one, None),
        ("beam_temperature", "beam", dict(opts=_opts(b, 0.5)), one, None),
        # ---- the call itself
        ("null_context", "greedy", dict(ctx=None), None, None),
        ("no_model", "plain", dict(ctx=e.frontend.handle), None, None),
        ("not_finalised", "mel", dict(ctx=e.unfinal.handle), None, None),
        ("null_pcm", "greedy", dict(pcm=None), one, None),
        ("null_prompt", "plain", dict(prompts=None), one, None),
        ("null_tokens_out", "mel", dict(tokens_out=None), one, None),
        ("null_lens_out", "windows", dict(lens_out=None), one, None),
        ("pcm_dtype", "greedy", dict(pcm_dtype=7), one, None),
        ("B_0", "greedy", dict(B=0), one, None),
        ("window_base", "mel", dict(mel_base=np.array([0, -1], dtype=np.int64)), one, None),
        ("window_len", "mel", dict(mel_len=_i32(0, 3000)), one, None),
        ("window_seek", "ragged", dict(rag, seek=_i32(0, -1)), one, None),
        ("window_frames_0", "best_of", dict(n_frames=_i32(3000, 0)), one, None),
        ("window_frames_3001", "beam", dict(n_frames=_i32(3001, 1500)), one, None),
        ("window_past_end", "mel", dict(seek=_i32(0, 2000)), one, None),
        ("set_f32_path", "windows", {}, one, f32),
        ("set_other_model", "windows", dict(set=e.other_set.handle), one, None),
        ("set_rows_null_B", "windows", dict(B=1, rows=None), one, None),
        ("set_row_outside", "windows_beam", dict(rows=_i32(0, 2)), one, None),
        ("prompt_len_0", "ragged", dict(rag, prompt_len=_i32(3, 0)), one, None),
        ("prompt_len_4", "windows", dict(rag, prompt_len=_i32(4, 2)), one, None),
        ("context_full", "greedy", dict(max_new=447), one, None),
        ("n_prompt_0", "greedy", dict(n_prompt=0), one, None),
        ("max_new_0", "plain", dict(max_new=0), one, None),
        ("prompt_token_negative", "greedy", dict(prompts=_i32(SOT, -1)), one, None),
        ("prompt_token_vocab", "mel", dict(prompts=_i32(SOT, NO_TS, SOT, V)), one, None),
        ("prompt_token_ragged", "ragged", dict(rag, prompts=_i32(SOT, NO_TS, 5, SOT, V, -7)), one, None),
        ("eot_vocab", "greedy", dict(eot=V), one, None),
        ("budgets_size", "mel", {}, [1, 1, 1], None),
        ("sot_tail_0", "ragged", dict(rag, sot_tail=0, opts=_opts(b, ns=NS_TOK), no_speech_out=ns_out), one, None),
        ("sot_tail_3", "windows", dict(rag, sot_tail=3, opts=_opts(b, ns=NS_TOK), no_speech_out=ns_out), one, None),
        ("temperature_nan", "plain", dict(opts=_opts(b, float("nan"))), one, None),
        ("temperature_negative", "mel", dict(opts=_opts(b, -0.5)), one, None),
        ("temperature_inf", "best_of", dict(opts=_opts(b, float("inf"))), one, None),
        ("temperature_tiny", "plain", dict(opts=_opts(b, 1e-39)), one, None),
        ("sot_index_negative", "plain", dict(opts=_opts(b, sot=-1)), one, None),
        ("sot_index_2", "mel", dict(opts=_opts(b, sot=2)), one, None),
        ("no_speech_token_low", "plain", dict(opts=_opts(b, ns=-2)), one, None),
        ("no_speech_token_vocab", "mel", dict(opts=_opts(b, ns=V)), one, None),
        ("no_speech_out_without_token", "plain", dict(no_speech_out=ns_out), one, None),
        ("repetition_f32_path", "mel", {}, one, rep_f32),
        ("lane_solo_cus_32", "mel", {}, one, solo),
        # ---- two checks at once: the order decides
        ("order_null_context_best_of", "best_of", dict(ctx=None, best_of=0), None, None),
        ("order_null_context_beam_size", "windows_beam", dict(ctx=None, beam_size=0), None, None),
        ("order_stride_not_finalised", "best_of", dict(ctx=e.unfinal.handle, prompt_stride=0), None, None),
        ("order_ragged_stride_not_finalised", "ragged", dict(rag, ctx=e.unfinal.handle, prompt_stride=0), None, None),
        ("order_beam_stride_not_finalised", "beam", dict(ctx=e.unfinal.handle, prompt_stride=0), None, None),
        ("order_window_prompt_token", "mel", dict(n_frames=_i32(3000, 0), prompts=_i32(SOT, NO_TS, SOT, V)), one, None),
        ("order_budgets_eot", "mel", dict(eot=V), [1, 1, 1], None),
        ("order_sot_tail_temperature", "ragged", dict(rag, sot_tail=3, opts=_opts(b, -1.0, ns=NS_TOK), no_speech_out=ns_out), one, None),
        ("order_mel_null_not_finalised", "mel", dict(ctx=e.unfinal.handle, mel=None), None, None),
        ("order_best_of_B_window", "best_of", dict(B=0, n_frames=_i32(0, 0)), one, None),
        ("order_dtype_B", "greedy", dict(pcm_dtype=7, B=0), one, None),
        ("order_eot_temperature", "plain", dict(eot=V, opts=_opts(b, -1.0)), one, None),
    ]
    assert len({c[0] for c in out}) == len(out)
    return out


def run_cases(e):
    """{name: [status, message, lens of the valid call that followed (null: the call was not on the model's context)]}"""
    got = {}
    for name, entry, over, budgets, setup in cases(e):
        if setup:
            setup[0]()
        try:
            if budgets:
                e.ctx.set_token_budgets(budgets)
            got[name] = e.call(entry, **over)
        finally:
            if setup:
                setup[1]()
        got[name].append(e.follow_up() if budgets else None)
    return got


@pytest.fixture(scope="module")
def results(pkg):
    e = Env(pkg.binding)
    try:
        assert e.follow_up() == [NEW, NEW]
        yield run_cases(e)
    finally:
        e.close()


def test_every_check_fails_as_on_the_parent(results):
    with open(GOLDEN_FILE) as f:
        want = json.load(f)
    assert sorted(results) == sorted(want)
    for name in want:
        print("%-36s %d %s" % (name, results[name][0], results[name][1]))
    bad = {n: (results[n][:2], want[n]) for n in want if results[n][:2] != want[n]}
    assert not bad, bad
    assert all(st != 0 for st, _ in want.values())


def test_a_failed_call_consumes_its_budgets(results):
    armed = {n: r[2] for n, r in results.items() if r[2] is not None and r[2] != [NEW, NEW]}
    assert not armed, "budgets survived a failed call: %r" % armed
    assert sum(r[2] is not None for r in results.values()) >= 60
