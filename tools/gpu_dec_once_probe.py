"""Launch times of the decode kernels whose text csrc/dec_kernels.hip states once, for A/B runs of two
builds of the library: run it alternately with and without WM_LIB_PATH / WM_DBG_LIB_PATH in ONE job, one process per run.

    python tools/gpu_dec_once_probe.py [rows,...]     (default 1,8,56,128)

Large-v2 width, heads and vocabulary with 2 encoder and 2 decoder layers, synthetic lively weights (seed 3), one decode group per
call (wm_set_lanes(1)), prompt of 3 tokens, 16 new tokens, eot = -1, timestamp rules on.  Per rows and mode one warm-up call,
then three calls under Context.profile() (eager launches, a HIP event pair round every launch): us per launch of
  plain      wm_transcribe_mel without options          dec_gemv_ln_logits      + dec_attn_self, dec_attn_cross / dec_attn_cross_fq
  extended   temperature 0.7 with a no-speech token      dec_gemv_ln_logits_x
  ext+rep    extended + repetition rules                 dec_gemv_ln_logits_xr
  ext+bias   extended + repetition rules + a bias table  dec_gemv_ln_logits_xb
  cand       wm_transcribe_mel_best_of, 16 windows x 5   dec_attn_cross_cand
and wmdbg_bench_dec_attention (graph-free back-to-back launches over 8 cache slices) at 8 and 56 rows: 448 and 1500 keys.
Prints one JSON line per figure."""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
EOT, TS0, NS_TOK, NEW = 50257, 50364, 50362, 16
rows_list = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 8, 56, 128]
dims = dict(b.MODEL_DIMS["large-v2"], n_audio_layer=2, n_text_layer=2)
ctx = b.Context(dims, debug=True)
ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
ctx.finalize()
ctx.set_lanes(1)
ctx.set_timestamp_rules(True, TS0, EOT, 50)
t = np.arange(480000) / 16000.0
pcm = np.stack([(0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t)).astype(np.float32) for i in range(8)])
mel = ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32)
SCOPES = ("dec_gemv_ln_logits", "dec_attn_self", "dec_attn_cross")


def win(B):
    return mel, (np.arange(B, dtype=np.int64) % 8) * (dims["n_mels"] * 3000), 3000, 0, 400


def profiled(case, rows, call):
    call()
    ctx.profile_enable(True)
    runs = {}
    for _ in range(3):
        ctx.profile_reset()
        call()
        for q, v in ctx.profile().items():
            if isinstance(v, dict) and v.get("n") and q.startswith(SCOPES):
                runs.setdefault(q, []).append(round(v["ms"] / v["n"] * 1e3, 2))
    ctx.profile_enable(False)
    for q, v in runs.items():
        print(json.dumps(dict(case=case, rows=rows, scope=q, us=v)), flush=True)


for B in rows_list:
    pr = np.tile(np.array([50258, 50259, 50359], np.int32), (B, 1))
    profiled("plain", B, lambda: ctx.transcribe_mel_raw(*win(B), pr, NEW, -1, None, logprobs=False))
    ext = lambda: ctx.transcribe_mel(*win(B), pr, NEW, eot=-1, temperature=0.7, seed=11, no_speech_token=NS_TOK)   # noqa: E731
    profiled("extended", B, ext)
    ctx.set_repetition_rules(1.3, 2, EOT)
    profiled("ext+rep", B, ext)
    ctx.set_sequence_bias({(7 * i + 5,): 1.5 for i in range(64)}, eot=EOT)
    profiled("ext+bias", B, ext)
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()
pr = np.tile(np.array([50258, 50259, 50359], np.int32), (16, 1))
profiled("cand", 80, lambda: ctx.transcribe_mel_best_of(*win(16), pr, NEW, 5, eot=-1, temperature=1.0, seed=11))
us = ctypes.c_float()
for B in (8, 56):
    for nk in (448, 1500):
        for rep in range(3):
            assert ctx.lib.wmdbg_bench_dec_attention(ctx.handle, B, 20, nk, nk, 1, 8, 200, ctypes.byref(us)) == 0
            print(json.dumps(dict(case="bench_dec_attention", rows=B, scope="keys %d" % nk, us=[round(us.value, 2)])), flush=True)
ctx.close()
