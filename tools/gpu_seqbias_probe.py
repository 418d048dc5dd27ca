"""Measurements of the sequence bias (wm_set_sequence_bias).

    python tools/gpu_seqbias_probe.py cost [model] [rows] [new]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), `new` tokens (default 224), no
        early stop, log-probs requested in every run so all take the extended (X) path: wall time of wm_transcribe with the
        table off and with
          t8       8 entries: four 3-token phrases with bias 2.0 and four banned 2-token sequences
          phrases  4096 entries: 1360 boosted 3-token phrases over 16 first tokens (1360 + 16 + 1360 prefixes) and 1360
                   banned 2-token sequences -- 4096 after expansion, 4096 distinct last tokens, 16 entries without a context
          singles  4096 single-token entries with bias 0.0: EVERY entry matches EVERY row at every position, so every row's
                   list holds 4096 ids and 4096 lanes per row look their total up -- the most the table can cost
        alternating, three runs each after a warm-up of each; the difference per decode position against off; then the
        HIP-event profile of one 16-token call per setting: wm_repeat_state, wm_seqbias_state and the logits launch alone.
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


def tables():
    t8 = {(1000 + i, 2000 + i, 3000 + i): 2.0 for i in range(4)}
    t8.update({(4000 + i, 5000 + i): -float("inf") for i in range(4)})
    phrases = {(100 + i % 16, 1000 + i // 16 * 16 + i % 16, 10000 + i): 2.0 for i in range(1360)}
    boost = list(phrases)
    phrases.update({(20000 + i, 30000 + i): -float("inf") for i in range(1360)})
    singles = {(7 * i + 5,): 0.0 for i in range(4096)}
    return {"off": (None, ()), "t8": (t8, ()), "phrases": (phrases, boost), "singles": (singles, ())}


def cost(name, rows, new):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    eot = 50257
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258, 50259, 50359]
    runs = tables()
    wall = {k: [] for k in runs}
    for k, (t, boost) in runs.items():       # warm-up of each: graph capture
        ctx.set_sequence_bias(t, boost, eot=eot)
        ctx.transcribe(pcm, prompt, new)
    for _ in range(3):
        for k, (t, boost) in runs.items():
            ctx.set_sequence_bias(t, boost, eot=eot)
            t0 = time.perf_counter()
            ctx.transcribe(pcm, prompt, new)
            wall[k].append(round(time.perf_counter() - t0, 5))
    positions = len(prompt) + new - 1
    off = min(wall["off"])
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us={k: round(min(v) / positions * 1e6, 2) for k, v in wall.items()},
               cost_us_per_position={k: round((min(v) - off) / positions * 1e6, 2) for k, v in wall.items() if k != "off"},
               cost_percent={k: round(100 * (min(v) - off) / off, 2) for k, v in wall.items() if k != "off"})
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    for k, (t, boost) in runs.items():
        ctx.set_sequence_bias(t, boost, eot=eot)
        ctx.transcribe(pcm, prompt, 16)
        ctx.profile_reset()
        ctx.transcribe(pcm, prompt, 16)
        prof = ctx.profile()
        fam[k] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                  if isinstance(v, dict) and v.get("n") and ("logits" in q or "repeat" in q or "seqbias" in q or "argmax" in q)}
    out["profile_us_per_launch"] = fam
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    ctx.profile_enable(False)
    ctx.set_sequence_bias(None)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "cost":
        raise SystemExit(__doc__)
    cost(sys.argv[2] if len(sys.argv) > 2 else "large-v2", int(sys.argv[3]) if len(sys.argv) > 3 else 56,
         int(sys.argv[4]) if len(sys.argv) > 4 else 224)
