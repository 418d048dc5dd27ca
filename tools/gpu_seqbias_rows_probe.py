"""Measurements of the row tables (wm_set_sequence_bias_tables / wm_set_bias_rows).

    python tools/gpu_seqbias_rows_probe.py cost [model] [rows] [new]
        As tools/gpu_seqbias_probe.py cost: synthetic lively weights of `model` (default large-v2) x `rows` chunks (default
        56), `new` tokens (default 224), no early stop, log-probs requested in every run so all take the extended (X) path.
        Wall time of wm_transcribe with the bias off and, at two table sizes, with ONE table for all rows (the existing path:
        the reference) against a table of the same size PER ROW:
          t8 / rows_t8            8 entries: four 3-token phrases with bias 2.0 and four banned 2-token sequences (row r's
                                  table: the same shifted by r ids, so the tables differ)
          singles / rows_singles  4096 single-token entries with bias 0.0: every entry matches its row at every position --
                                  16 tables of 4096 fill the pool, so the rows share 16 full tables (row r: table r % 16)
        alternating, three runs each after a warm-up of each; the difference per decode position against off and against the
        single table of the same size; then the HIP-event profile of one 16-token call per setting: wm_repeat_state, the
        bias state launch (wm_seqbias_state / wm_seqbias_rows_state) and the logits launch alone.
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
POOL = 65536


def t8(shift):
    t = {(1000 + i + shift, 2000 + i + shift, 3000 + i + shift): 2.0 for i in range(4)}
    t.update({(4000 + i + shift, 5000 + i + shift): -float("inf") for i in range(4)})
    return t


def singles(shift):
    return {(7 * i + 5 + shift,): 0.0 for i in range(4096)}


def settings(rows):
    """name -> (single table or None, tables or None, row map or None)"""
    n_full = min(rows, POOL // 4096)
    return {"off": (None, None, None),
            "t8": (t8(0), None, None),
            "rows_t8": (None, [t8(r) for r in range(rows)], list(range(rows))),
            "singles": (singles(0), None, None),
            "rows_singles": (None, [singles(r % 7) for r in range(n_full)], [r % n_full for r in range(rows)])}


def apply(ctx, setting, eot):
    one, tables, rows = setting
    if tables is not None:
        ctx.set_sequence_bias_tables(tables, eot=eot)
    else:
        ctx.set_sequence_bias(one, eot=eot)      # (replaces the tables; None clears both)
    return rows


def cost(name, rows, new):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    eot = 50257
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258, 50259, 50359]
    runs = settings(rows)

    def call(k, n):
        m = apply(ctx, runs[k], eot)
        if m is not None:
            ctx.set_bias_rows(m)
        t0 = time.perf_counter()
        ctx.transcribe(pcm, prompt, n)
        return time.perf_counter() - t0
    wall = {k: [] for k in runs}
    for k in runs:       # warm-up of each: graph capture
        call(k, new)
    for _ in range(3):
        for k in runs:
            wall[k].append(round(call(k, new), 5))
    positions = len(prompt) + new - 1
    best = {k: min(v) for k, v in wall.items()}
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us={k: round(v / positions * 1e6, 2) for k, v in best.items()},
               cost_us_per_position={k: round((v - best["off"]) / positions * 1e6, 2) for k, v in best.items() if k != "off"},
               rows_minus_single_us_per_position={k: round((best["rows_" + k] - best[k]) / positions * 1e6, 2) for k in ("t8", "singles")})
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    for k in runs:
        call(k, 16)
        ctx.profile_reset()
        call(k, 16)
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
