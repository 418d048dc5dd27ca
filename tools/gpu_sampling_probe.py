"""Measurements of the sampling rules (wm_set_sampling_rules).

    python tools/gpu_sampling_probe.py effect
        The `lively` tiny model of tests/test_model_gpu.py on tones(8), prompt [10, 21, 5], 32 tokens, eot 890: the window
        decodes (rows over all steps) a transcribe_with_fallback run makes without the rules and with (50, 0.9, 0), and the
        rows that still need fallback at the end.

    python tools/gpu_sampling_probe.py cost [model] [rows] [new]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), `new` tokens (default 224), no
        early stop, sampling at T = 1 in both runs: wall time of wm_transcribe with the rules off and with (50, 0.9, 0.05),
        alternating, three runs each after a warm-up of each; the difference per decode position; then the HIP-event profile
        of one call each: the truncation launch and the logits launch (which stores the f32 row with the rules on) alone.
        A last pair times (V + 7, 1, 0): nothing is cut, every id is drawn a second time -- the kernel's longest draw pass.
Prints JSON lines."""
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


def effect():
    from oracle import whisper_ref as R
    from test_model_gpu import LIVELY_GAIN, nontrivial_ln, tones
    dims = dict(R.TINY_DIMS)
    sd = nontrivial_ln(W.synthetic_state_dict(dims, seed=11))
    for k in sd:
        if sd[k].ndim >= 2 and "positional" not in k:
            sd[k] = sd[k] * np.float32(LIVELY_GAIN)
    ctx = b.Context(dims)
    ctx.load_state_dict(sd)
    ctx.finalize()
    pcm, prompt, new, eot = tones(8), [10, 21, 5], 32, 890
    for name, kw in (("rules off", {}), ("(50, 0.9, 0)", dict(top_k=50, top_p=0.9)), ("(8, 0.9, 0)", dict(top_k=8, top_p=0.9))):
        for thr in (-1.0, -4.0):
            fb = ctx.transcribe_with_fallback(pcm, prompt, new, eot, logprob_threshold=thr, seed=3, **kw)
            print(json.dumps(dict(setting=name, logprob_threshold=thr, fallback_steps=[(s[0], len(s[2])) for s in fb["steps"]],
                                  window_decodes=int(sum(len(s[2]) for s in fb["steps"])),
                                  final_temperature=fb["temperature"].tolist(),
                                  avg_logprob=[round(float(x), 3) for x in fb["avg_logprob"]],
                                  still_needed=int(fb["needs_fallback"].sum()))))
    ctx.close()


def cost(name, rows, new):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    V = dims["n_vocab"]
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258, 50259, 50359]
    runs = {"off": (0, 1.0, 0.0), "on": (50, 0.9, 0.05), "keep_all": (V + 7, 1.0, 0.0)}
    wall = {k: [] for k in runs}
    for k, st in runs.items():       # warm-up of each: graph capture
        ctx.set_sampling_rules(*st)
        ctx.transcribe(pcm, prompt, new, temperature=1.0, seed=5)
    for _ in range(3):
        for k, st in runs.items():
            ctx.set_sampling_rules(*st)
            t0 = time.perf_counter()
            ctx.transcribe(pcm, prompt, new, temperature=1.0, seed=5)
            wall[k].append(round(time.perf_counter() - t0, 5))
    positions = len(prompt) + new - 1
    per = {k: min(v) / positions * 1e6 for k, v in wall.items()}
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us={k: round(v, 2) for k, v in per.items()},
               rules_cost_us_per_position=round(per["on"] - per["off"], 2),
               rules_cost_percent=round(100 * (per["on"] - per["off"]) / per["off"], 2),
               keep_all_cost_us_per_position=round(per["keep_all"] - per["off"], 2))
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    for k, st in runs.items():
        ctx.set_sampling_rules(*st)
        ctx.transcribe(pcm, prompt, 16, temperature=1.0, seed=5)
        ctx.profile_reset()
        ctx.transcribe(pcm, prompt, 16, temperature=1.0, seed=5)
        prof = ctx.profile()
        fam[k] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                  if isinstance(v, dict) and v.get("n") and ("logits" in q or "sample_trunc" in q or "argmax" in q)}
    out["profile_us_per_launch"] = fam
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    ctx.profile_enable(False)
    ctx.set_sampling_rules()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cost":
        cost(sys.argv[2] if len(sys.argv) > 2 else "large-v2", int(sys.argv[3]) if len(sys.argv) > 3 else 56,
             int(sys.argv[4]) if len(sys.argv) > 4 else 224)
    else:
        effect()
