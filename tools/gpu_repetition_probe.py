"""Measurements of the repetition rules (wm_set_repetition_rules).

    python tools/gpu_repetition_probe.py effect
        The `lively` tiny model of tests/test_model_gpu.py on tones(4), prompt [1, 2, 3], 32 tokens, eot 1000: repeated
        3-grams per row, distinct tokens and compression_ratio_tokens for plain greedy, (1.0, 3) and (1.5, 0), and the steps a
        transcribe_with_fallback run takes in each case (compression-ratio rule only: logprob_threshold None).

    python tools/gpu_repetition_probe.py cost [model] [rows] [new]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), `new` tokens (default 224), no
        early stop, log-probs requested in both runs so both take the extended (X) path: wall time of wm_transcribe with the
        rules off and with (1.3, 3), alternating, three runs each after a warm-up of each; the difference per decode
        position; then the HIP-event profile of one call with the rules on: wm_repeat_state and the logits launch alone.
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
    import repeat_ref as RR
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
    pcm, prompt, new, eot = tones(4), [1, 2, 3], 32, 1000
    for name, (p, n) in (("plain", (1.0, 0)), ("no_repeat_ngram_size=3", (1.0, 3)), ("repetition_penalty=1.5", (1.5, 0)),
                         ("(1.3, 3)", (1.3, 3))):
        ctx.set_repetition_rules(p, n, eot)
        t, l = ctx.transcribe_greedy(pcm, prompt, new, eot=eot)
        fb = ctx.transcribe_with_fallback(pcm, prompt, new, eot, logprob_threshold=None)
        print(json.dumps(dict(setting=name, lens=l.tolist(),
                              repeated_3grams=[RR.repeated_ngrams(t[i, :l[i]], 3, eot) for i in range(4)],
                              distinct_tokens=[len(set(t[i, :l[i]].tolist())) for i in range(4)],
                              compression_ratio_tokens=[round(b.compression_ratio_tokens(t[i, :l[i]], dims["n_vocab"]), 3) for i in range(4)],
                              fallback_steps=[(s[0], len(s[2])) for s in fb["steps"]],
                              fallback_final_temperature=fb["temperature"].tolist(),
                              fallback_still_needed=fb["needs_fallback"].tolist())))
    ctx.set_repetition_rules()
    ctx.close()


def cost(name, rows, new):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    eot = 50257
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258, 50259, 50359]
    runs = {"off": (1.0, 0), "on": (1.3, 3)}
    wall = {k: [] for k in runs}
    for k, (p, n) in runs.items():       # warm-up of each: graph capture
        ctx.set_repetition_rules(p, n, eot)
        ctx.transcribe(pcm, prompt, new)
    for _ in range(3):
        for k, (p, n) in runs.items():
            ctx.set_repetition_rules(p, n, eot)
            t0 = time.perf_counter()
            ctx.transcribe(pcm, prompt, new)
            wall[k].append(round(time.perf_counter() - t0, 5))
    positions = len(prompt) + new - 1
    d_us = (min(wall["on"]) - min(wall["off"])) / positions * 1e6
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us=dict(off=round(min(wall["off"]) / positions * 1e6, 2), on=round(min(wall["on"]) / positions * 1e6, 2)),
               rules_cost_us_per_position=round(d_us, 2), rules_cost_percent=round(100 * d_us / (min(wall["off"]) / positions * 1e6), 2))
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    for k, (p, n) in runs.items():
        ctx.set_repetition_rules(p, n, eot)
        ctx.transcribe(pcm, prompt, 16)
        ctx.profile_reset()
        ctx.transcribe(pcm, prompt, 16)
        prof = ctx.profile()
        fam[k] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                  if isinstance(v, dict) and v.get("n") and ("logits" in q or "repeat" in q or "argmax" in q)}
    out["profile_us_per_launch"] = fam
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    ctx.profile_enable(False)
    ctx.set_repetition_rules()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cost":
        cost(sys.argv[2] if len(sys.argv) > 2 else "large-v2", int(sys.argv[3]) if len(sys.argv) > 3 else 56,
             int(sys.argv[4]) if len(sys.argv) > 4 else 224)
    else:
        effect()
