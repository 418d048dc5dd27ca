"""Measurements of the alternatives request (wm_request_alternatives).

    python tools/gpu_alternatives_probe.py [model] [rows] [new]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), `new` tokens (default 64), no
        early stop, arg-max decode with log-probs in every run: wall time of wm_transcribe without a request and with a
        request of n = 1, 5 and 16, alternating, three runs each after a warm-up of each; the difference per decode position;
        then the HIP-event profile of one 16-token call each: the alternatives launch, the logits launch (which stores the f32
        row with a request) and the arg-max close alone.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding


def cost(name, rows, new):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258, 50259, 50359]
    runs = {"none": None, "n1": 1, "n5": 5, "n16": 16}
    wall = {k: [] for k in runs}
    for n in runs.values():       # warm-up of each: graph capture (one graph serves every n: the second and later are replays)
        ctx.transcribe(pcm, prompt, new, alternatives=n)
    for _ in range(3):
        for k, n in runs.items():
            t0 = time.perf_counter()
            ctx.transcribe(pcm, prompt, new, alternatives=n)
            wall[k].append(round(time.perf_counter() - t0, 5))
    positions = len(prompt) + new - 1
    per = {k: min(v) / positions * 1e6 for k, v in wall.items()}
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us={k: round(v, 2) for k, v in per.items()},
               request_cost_us_per_position={k: round(per[k] - per["none"], 2) for k in runs if k != "none"},
               request_cost_percent={k: round(100 * (per[k] - per["none"]) / per["none"], 2) for k in runs if k != "none"})
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    for k, n in runs.items():
        ctx.transcribe(pcm, prompt, 16, alternatives=n)
        ctx.profile_reset()
        ctx.transcribe(pcm, prompt, 16, alternatives=n)
        prof = ctx.profile()
        fam[k] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                  if isinstance(v, dict) and v.get("n") and ("logits" in q or "alternatives" in q or "argmax" in q)}
    out["profile_us_per_launch"] = fam
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    ctx.profile_enable(False)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    cost(sys.argv[1] if len(sys.argv) > 1 else "large-v2", int(sys.argv[2]) if len(sys.argv) > 2 else 56,
         int(sys.argv[3]) if len(sys.argv) > 3 else 64)
