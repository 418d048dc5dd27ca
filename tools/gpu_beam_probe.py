"""Cost of beam search: wm_transcribe_mel_beam against wm_transcribe_mel_best_of of the same build on the same windows.  The two
calls decode the same rows (windows x 5) with the same cross-K/V sharing, so the difference is the beam tail: the f32 logits
store, the per-row list kernel, the per-window step and the re-parenting of the self-attention cache.  Synthetic lively
weights of the model given as argv[1] (default large-v2), eot = -1 (fixed length), 224 new tokens, width 5 (--width N), at 8
windows (--windows 8,24).

    python tools/gpu_beam_probe.py [model] [--mode beam | best_of] [--runs 3] [--new 224] [--windows 8]

Prints one JSON line per (windows, run): wall seconds, wm_last_stage_ms (front end / encoder + cross K/V / decode) and the
per-position time.  --profile adds one profiled (eager, one lane) call per size and prints the per-family times of the three
beam kernels: beam_topk, beam_select, beam_reorder."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


profile = "--profile" in sys.argv
if profile:
    sys.argv.remove("--profile")
mode = _opt("--mode", "beam")
runs = int(_opt("--runs", "3"))
NEW = int(_opt("--new", "224"))
N = int(_opt("--width", "5"))
windows = [int(x) for x in _opt("--windows", "8").split(",")]
name = sys.argv[1] if len(sys.argv) > 1 else "large-v2"
dims = dict(b.MODEL_DIMS[name])
SOT, TASK = 50258, 50359
PROMPT = [SOT, 50259, TASK]

ctx = b.Context(dims)
ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
ctx.finalize()
n_mels = dims["n_mels"]
pcm = np.zeros((max(windows), 480000), np.float32)
t = np.arange(480000) / 16000.0
for i in range(pcm.shape[0]):
    pcm[i] = 0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (0.2 + 0.05 * i) * t))
mel = ctx.logmel(pcm, n_mels=n_mels, out_dtype=np.float32)
d_mel = ctx.to_device(mel)
positions = len(PROMPT) + NEW - 1


def run(B):
    base = np.arange(B, dtype=np.int64) * (n_mels * 3000)
    prompts = np.tile(np.array(PROMPT, np.int32), (B, 1))
    t0 = time.perf_counter()
    if mode == "beam":
        r = ctx.transcribe_mel_beam(d_mel, base, 3000, 0, 3000, prompts, NEW, N, eot=-1, mem=b.WM_MEM_DEVICE)
    else:
        r = ctx.transcribe_mel_best_of(d_mel, base, 3000, 0, 3000, prompts, NEW, N, eot=-1, temperature=1.0, seed=11,
                                       sample_ids=np.arange(B, dtype=np.uint32), mem=b.WM_MEM_DEVICE)
    wall = time.perf_counter() - t0
    st = [float(x) for x in ctx.last_stage_ms()]
    distinct = int(np.mean([len({tuple(c) for c in r.tokens[w]}) for w in range(B)]) * 100) / 100.0
    return dict(model=name, mode=mode, windows=B, width=N, new=NEW, wall_s=round(wall, 4), stage_ms=[round(x, 3) for x in st],
                per_position_ms=round(st[2] / positions, 4), distinct_rows_per_window=distinct)


try:
    for B in windows:
        run(B)   # warm-up: buffers, lanes, the position graphs
        for k in range(runs):
            print(json.dumps(dict(run(B), run=k)), flush=True)
        if profile:
            ctx.profile_reset()
            ctx.profile_enable(True)
            try:
                run(B)
                p = ctx.profile()
            finally:
                ctx.profile_enable(False)
            fams = {k: dict(n=v["n"], ms=round(v["ms"], 3), us_each=round(1000.0 * v["ms"] / max(v["n"], 1), 2))
                    for k, v in p.items() if k.startswith("beam_") or k in ("dec_attn_cross_cand", "dec_attn_self", "dec_gemv")}
            print(json.dumps(dict(model=name, mode=mode, windows=B, width=N, profiled_families=fams)), flush=True)
finally:
    ctx.dev_free(d_mel)
    ctx.close()
