"""The decode paths' outputs as digests: one sha256 per case over the raw bytes of everything the call returns, to compare two
builds of the library bit for bit (the suite ties the paths to each other, not to the commit before).

    python tools/gpu_decode_bits.py                                        (this build)
    WM_LIB_PATH=... WM_DBG_LIB_PATH=... python tools/gpu_decode_bits.py    (another build), then diff the two outputs

Synthetic lively weights only.  decode_logits at tiny and base geometry (1, 8, 17 rows, T = 9, teacher panel 1 and 8); every
transcribe entry on a model of large-v2 width, heads and vocabulary with 2 encoder and 2 decoder layers, one decode group per call
(wm_set_lanes(1)), at 1, 8 and 24 windows: 8 rows x 20 heads is the fused query + cross-attention launch, 24 rows the streaming
one -- the first lines print the launch plan (wmdbg_dec_attn_plan) to show it.  Prints `case digest` lines."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
SOT, EOT, TS0, NS_TOK = 50258, 50257, 50364, 50362
PROMPT = [SOT, 50259, 50359]
NEW = 12


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def say(case, *arrays):
    print("%-44s %s" % (case, digest(*arrays)), flush=True)


def model(dims, seed):
    ctx = b.Context(dims)
    ctx.init_synthetic(seed, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    return ctx


def plans(H, d):
    lib = b.load_debug_library()
    ip = ctypes.POINTER(ctypes.c_int32)
    lib.wmdbg_dec_attn_plan.argtypes = [ip, ctypes.c_int, ip]
    lib.wmdbg_dec_attn_plan.restype = ctypes.c_int

    def plan(form, B, nsplit):
        a = np.zeros((1, 16), np.int32)
        a[0, :13] = [form, B, 0, 0, H, 1500, 1500, nsplit, d, 2, 0, 0, 256]
        out = np.zeros((1, 16), np.int32)
        assert lib.wmdbg_dec_attn_plan(a.ctypes.data_as(ip), 1, out.ctypes.data_as(ip)) == 1
        return out[0]
    for B in (1, 8, 24):
        ns = int(plan(0, B, 1)[14])
        print("plan: %2d rows x %d heads: fused query applies %d; cross-attention variant %d at nsplit %d"
              % (B, H, plan(2, B, 1)[14], plan(0, B, ns)[1], ns), flush=True)


def logits_cases():
    rng = np.random.default_rng(7)
    for name in ("tiny.en", "base"):
        dims = dict(b.MODEL_DIMS[name])
        ctx = model(dims, 3)
        for B in (1, 8, 17):
            xa = rng.standard_normal((B, dims["n_audio_ctx"], dims["n_audio_state"])).astype(np.float32)
            toks = rng.integers(0, dims["n_vocab"], (B, 9)).astype(np.int32)
            for w in (1, 8):
                ctx.set_teacher_panel(w)
                say("decode_logits %s rows %d panel %d" % (name, B, w), ctx.decode_logits(toks, xa))
        ctx.set_teacher_panel(1)
        ctx.close()


def tone_mel(ctx, dims, n):
    t = np.arange(480000) / 16000.0
    pcm = np.stack([(0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (0.2 + 0.05 * i) * t))).astype(np.float32)
                    for i in range(n)])
    return ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32)


def result(r):
    return [getattr(r, k, None) for k in ("tokens", "lens", "logprobs", "no_speech_prob", "best", "start_frames", "stats")]


def transcribe_cases():
    dims = dict(b.MODEL_DIMS["large-v2"], n_audio_layer=2, n_text_layer=2)
    plans(dims["n_text_head"], dims["n_text_state"])
    ctx = model(dims, 3)
    ctx.set_lanes(1)
    draft = model(dict(b.MODEL_DIMS["tiny.en"], n_vocab=dims["n_vocab"], n_audio_layer=1, n_text_layer=1), 5)
    mel = tone_mel(ctx, dims, 24)
    stride = dims["n_mels"] * 3000

    def win(B):
        return mel, np.arange(B, dtype=np.int64) * stride, 3000, 0, 3000

    def rules(on, c=ctx):
        c.set_suppress(list(range(EOT + 1, TS0)) if on else [], [EOT] if on else [])
        c.set_timestamp_rules(on, TS0, EOT, 50)

    for B in (1, 8, 24):
        pr = np.tile(np.array(PROMPT, np.int32), (B, 1))
        ids = np.arange(B, dtype=np.uint32)
        say("transcribe_mel greedy rows %d" % B, *ctx.transcribe_mel_raw(*win(B), pr, NEW, -1, None, logprobs=False))
        rules(True)
        say("transcribe_mel greedy+rules rows %d" % B, *ctx.transcribe_mel_raw(*win(B), pr, NEW, -1, None, logprobs=False))
        say("transcribe_mel rules T=0.7 no_speech rows %d" % B,
            *result(ctx.transcribe_mel(*win(B), pr, NEW, eot=-1, temperature=0.7, seed=11, no_speech_token=NS_TOK, sample_ids=ids)))
        rules(False)
        say("transcribe_mel T=0 logprobs rows %d" % B, *result(ctx.transcribe_mel(*win(B), pr, NEW, eot=-1)))
        ctx.set_repetition_rules(1.3, 2, EOT)
        say("transcribe_mel repetition rows %d" % B, *result(ctx.transcribe_mel(*win(B), pr, NEW, eot=-1, no_speech_token=NS_TOK)))
        ctx.set_sequence_bias({(7 * i + 5,): 1.5 for i in range(64)} | {(100 + i, 200 + i): -float("inf") for i in range(8)}, eot=EOT)
        say("transcribe_mel repetition+bias rows %d" % B, *result(ctx.transcribe_mel(*win(B), pr, NEW, eot=-1, temperature=0.7, seed=5)))
        ctx.set_sequence_bias(None)
        ctx.set_repetition_rules()
        ragged = [[50361] + [1000 + 3 * j for j in range(i % 4)] + PROMPT for i in range(B)]
        say("transcribe_mel ragged prompts rows %d" % B, *result(ctx.transcribe_mel(*win(B), ragged, NEW, eot=-1, no_speech_token=NS_TOK, sot_tail=3)))
        # early stop: a row ends at its budget (or at <|endoftext|>), leaves the live list, and the rest of the group goes on
        say("transcribe_mel early stop + budgets rows %d" % B,
            *result(ctx.transcribe_mel(*win(B), pr, NEW, eot=EOT, budgets=[2 + (5 * i) % (NEW - 1) for i in range(B)])))
    pr = np.tile(np.array(PROMPT, np.int32), (16, 1))
    for N, B in ((5, 16), (6, 4)):
        say("transcribe_mel_best_of %d windows %d" % (N, B), *result(ctx.transcribe_mel_best_of(
            *win(B), pr[:B], NEW, N, eot=-1, temperature=1.0, seed=11, no_speech_token=NS_TOK, sample_ids=np.arange(B, dtype=np.uint32))))
    r = ctx.transcribe_mel_beam(*win(8), pr[:8], NEW, 5, eot=EOT, no_speech_token=NS_TOK)
    hyp = [x[w, :r.n_hyp[w]] for w in range(8) for x in (r.tokens, r.lens, r.sum_logprob, r.logprobs)]   # (the filled slots)
    say("transcribe_mel_beam 5 windows 8", r.n_hyp, r.best, r.no_speech_prob, *hyp)
    say("transcribe_mel_aligned windows 8", *result(ctx.transcribe_mel_aligned(*win(8), pr[:8], NEW, eot=-1, no_speech_token=NS_TOK)))
    rules(True)
    rules(True, draft)
    say("transcribe_mel_speculative draft_len 4 windows 8",
        *result(ctx.transcribe_mel_speculative(draft, *win(8), pr[:8], NEW, 4, eot=-1, no_speech_token=NS_TOK)))
    draft.close()
    ctx.close()


if __name__ == "__main__":
    logits_cases()
    transcribe_cases()
