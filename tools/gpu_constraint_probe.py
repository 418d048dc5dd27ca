"""Measurements of the constraint (wm_set_constraint).

    python tools/gpu_constraint_probe.py cost [model] [rows]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), a one-token prompt, no early stop,
        log-probs requested and the repetition rules ON (penalty 1 + 2^-23: the X path with `rep`, wm_repeat_state and the
        DE_LOGITS_XR epilogue) in every run, so the constraint's launch is the only difference.  The automaton is the two-state
        digit loop with eot and every id above it suppressed: every generated token is a text token, so a history of k tokens is
        a walk of k lookups -- the worst case.  For new = 8, 64 and 447 tokens: wall time of wm_transcribe off / on,
        alternating, three runs each after a warm-up of each, and the difference per decode position; then the HIP-event
        profile of one call per setting: wm_repeat_state, wm_constraint_state and the logits launch alone.  A call of `new`
        tokens averages the histories 0 .. new - 1, so the state launch's time is fitted as a + b * k over the three means and
        read at k = 8, 64 and 447.
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


def digit_loop():
    d = list(range(50, 60))
    return b.Constraint([0, 10, 20], d + d, [1] * 10 + [0] * 10, [-1, -1], [1, 0])


def cost(name, rows):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    eot, V = 50257, int(dims["n_vocab"])
    pcm = np.tile(tones(8), ((rows + 7) // 8, 1))[:rows]
    prompt = [50258]
    ctx.set_suppress(list(range(eot, V)), [])
    ctx.set_repetition_rules(float(np.float32(1.0) + np.float32(2.0 ** -23)), 0, eot)
    auto = digit_loop()

    def call(on, n):
        ctx.set_constraint(auto if on else None, eot=eot)
        t0 = time.perf_counter()
        r = ctx.transcribe(pcm, prompt, n)
        dt = time.perf_counter() - t0
        if on:
            assert np.all((r.tokens >= 50) & (r.tokens < 60)), "a row left the digit loop"
        return dt
    out = dict(model=name, rows=rows, runs={})
    means = {}
    for new in (8, 64, 447):
        wall = {False: [], True: []}
        for on in (False, True):      # warm-up of each: graph capture
            call(on, new)
        for _ in range(3):
            for on in (False, True):
                wall[on].append(round(call(on, new), 5))
        positions = len(prompt) + new - 1
        best = {k: min(v) for k, v in wall.items()}
        run = dict(positions=positions, wall_s=dict(off=wall[False], on=wall[True]),
                   per_position_us=dict(off=round(best[False] / positions * 1e6, 2), on=round(best[True] / positions * 1e6, 2)),
                   cost_us_per_position=round((best[True] - best[False]) / positions * 1e6, 2))
        ctx.profile_enable(True)      # per-family HIP-event times (eager launches: every launch bracketed by events)
        fam = {}
        for on in (False, True):
            call(on, new)
            ctx.profile_reset()
            call(on, new)
            prof = ctx.profile()
            fam["on" if on else "off"] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                                          if isinstance(v, dict) and v.get("n") and ("logits" in q or "repeat" in q or "constraint" in q)}
        run["profile_us_per_launch"] = fam
        run["profile_overhead_us"] = ctx.profile_overhead_us()
        ctx.profile_enable(False)
        means[(new - 1) / 2.0] = fam["on"].get("constraint_state", float("nan"))
        out["runs"][str(new)] = run
    ks, ts = np.array(sorted(means)), np.array([means[k] for k in sorted(means)])
    slope, icpt = np.polyfit(ks, ts, 1)
    out["state_launch_fit_us"] = dict(a=round(float(icpt), 2), b_per_token=round(float(slope), 4),
                                      at={str(k): round(float(icpt + slope * k), 2) for k in (8, 64, 447)})
    ctx.set_constraint(None)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "cost":
        raise SystemExit(__doc__)
    cost(sys.argv[2] if len(sys.argv) > 2 else "large-v2", int(sys.argv[3]) if len(sys.argv) > 3 else 56)
