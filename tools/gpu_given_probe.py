"""Measurements of given tokens (wm_set_given_tokens).

    python tools/gpu_given_probe.py [model] [rows] [new]
        Synthetic lively weights of `model` (default large-v2) x `rows` chunks (default 56), `new` tokens (default 64), no
        early stop, arg-max decode with log-probs in every run:
        1. wall time of wm_transcribe without a table and with every row given (the plain call's own tokens), alternating,
           three runs each after a warm-up of each; the difference per decode position;
        2. the HIP-event profile of one 16-token call each: the given-tokens launch, the logits launch (which stores the f32
           row for a group with a given row) and the arg-max close alone;
        3. score_given of 4 texts x 8 windows of 24 tokens through ONE best-of call against four plain window-set calls of 8
           rows each, alternating, three runs each after a warm-up of each.
    python tools/gpu_given_probe.py panel [model]
        Given panels (wm_set_given_panel): score_given of 4 texts x 8 windows of 24 tokens (+ eot) on
        synthetic lively weights of `model` (default large-v2): form="rows" at widths 1 / 2 / 4 / 8 and form="best_of",
        interleaved, three runs each after a warm-up of each, every result compared bit for bit with width 1; then one
        profiled call (every launch bracketed by an event pair, so the bracketing bias is included) at widths 1 and 8: the
        sum over all launches, the rounds, and the three panel launches alone.  On a tree without the setting (the parent
        commit) the same two paths run as that tree has them: score_given's best-of call and the plain call with the rows
        repeated.
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
    plain = ctx.transcribe(pcm, prompt, new)
    table = [[int(t) for t in row] for row in plain.tokens]
    runs = {"none": None, "given": table}
    wall = {k: [] for k in runs}
    for g in runs.values():       # warm-up of each: graph capture
        r = ctx.transcribe(pcm, prompt, new, given=g)
        assert np.array_equal(r.tokens, plain.tokens) and np.array_equal(r.logprobs.view(np.uint32), plain.logprobs.view(np.uint32))
    for _ in range(3):
        for k, g in runs.items():
            t0 = time.perf_counter()
            ctx.transcribe(pcm, prompt, new, given=g)
            wall[k].append(round(time.perf_counter() - t0, 5))
    positions = len(prompt) + new - 1
    per = {k: min(v) / positions * 1e6 for k, v in wall.items()}
    out = dict(model=name, rows=rows, new=new, positions=positions, wall_s=wall,
               per_position_us={k: round(v, 2) for k, v in per.items()},
               given_cost_us_per_position=round(per["given"] - per["none"], 2),
               given_cost_percent=round(100 * (per["given"] - per["none"]) / per["none"], 2))
    # per-family HIP-event times (eager launches: every launch bracketed by events)
    ctx.profile_enable(True)
    fam = {}
    short = [row[:16] for row in table]
    for k, g in (("none", None), ("given", short)):
        ctx.transcribe(pcm, prompt, 16, given=g)
        ctx.profile_reset()
        ctx.transcribe(pcm, prompt, 16, given=g)
        prof = ctx.profile()
        fam[k] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in prof.items()
                  if isinstance(v, dict) and v.get("n") and ("logits" in q or "given" in q or "argmax" in q)}
    out["profile_us_per_launch"] = fam
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    ctx.profile_enable(False)
    # score_given: 4 texts x 8 windows through one best-of call against four plain calls
    eot, K, n_text = 50257, 4, 24
    g = np.random.default_rng(7)
    texts = [[[int(t) for t in g.integers(0, eot, n_text)] for _ in range(K)] for _ in range(8)]
    mel = ctx.logmel(tones(8), out_dtype=np.float32)
    sw = {"best_of": [], "four_calls": []}
    with ctx.encode_windows(mel.reshape(-1), np.arange(8, dtype=np.int64) * dims["n_mels"] * 3000, 3000, 0, 3000) as ws:
        def best_of():
            return b.score_given(ctx, ws, None, prompt, texts, eot)

        def four_calls():
            res = []
            for k in range(K):
                given = [t[k] + [eot] for t in texts]
                res.append(ctx.transcribe_windows(ws, None, prompt, n_text + 1, eot=eot, budgets=[n_text + 1] * 8, given=given))
            return res
        one, four = best_of(), four_calls()
        for w_ in range(8):
            for k in range(K):
                assert np.array_equal(one.logprobs[w_][k].view(np.uint32), four[k].logprobs[w_].view(np.uint32))
        for _ in range(3):
            for k, f in (("best_of", best_of), ("four_calls", four_calls)):
                t0 = time.perf_counter()
                f()
                sw[k].append(round(time.perf_counter() - t0, 5))
    out["score_given_wall_s"] = sw
    out["score_given_best_of_over_four_calls"] = round(min(sw["best_of"]) / min(sw["four_calls"]), 3)
    ctx.close()
    print(json.dumps(out))


def panel(name):
    from test_model_gpu import tones
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
    ctx.finalize()
    has = hasattr(ctx, "set_given_panel")
    prompt = [50258, 50259, 50359]
    eot, K, n_text = 50257, 4, 24
    g = np.random.default_rng(7)
    texts = [[[int(t) for t in g.integers(0, eot, n_text)] for _ in range(K)] for _ in range(8)]
    mel = ctx.logmel(tones(8), out_dtype=np.float32)
    out = dict(model=name, windows=8, texts=K, tokens=n_text + 1, given_panel=has)
    with ctx.encode_windows(mel.reshape(-1), np.arange(8, dtype=np.int64) * dims["n_mels"] * 3000, 3000, 0, 3000) as ws:
        def rows_call():   # the plain call with the rows repeated: what score_given(form="rows") makes
            flat = [t + [eot] for ts in texts for t in ts]
            return ctx.transcribe_windows(ws, [w_ for w_ in range(8) for _ in range(K)], prompt, n_text + 1, eot=eot,
                                          budgets=[len(t) for t in flat], given=flat)

        def at(width):
            def f():
                ctx.set_given_panel(width)
                try:
                    return rows_call()
                finally:
                    ctx.set_given_panel(1)
            return f
        runs = {"best_of": lambda: b.score_given(ctx, ws, None, prompt, texts, eot).result}
        if has:
            for width in (1, 2, 4, 8):
                runs["rows_w%d" % width] = at(width)
        else:
            runs["rows_w1"] = rows_call
        base = runs["rows_w1"]()
        for k, f in runs.items():       # warm-up of each (graph capture), and the bits
            r = f()
            if k != "best_of":
                assert np.array_equal(r.tokens, base.tokens) and np.array_equal(r.logprobs.view(np.uint32), base.logprobs.view(np.uint32)), k
            else:
                assert np.array_equal(r.logprobs.reshape(base.logprobs.shape).view(np.uint32), base.logprobs.view(np.uint32))
        wall = {k: [] for k in runs}
        for _ in range(3):
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                wall[k].append(round(time.perf_counter() - t0, 5))
        out["wall_s"] = wall
        out["best_ms"] = {k: round(min(v) * 1e3, 2) for k, v in wall.items()}
        if has:
            ctx.profile_enable(True)
            prof = {}
            for width in (1, 8):
                at(width)()
                ctx.profile_reset()
                at(width)()
                pr = {q: v for q, v in ctx.profile().items() if isinstance(v, dict) and v.get("n")}
                prof["w%d" % width] = dict(total_ms=round(sum(v["ms"] for v in pr.values()), 3), launches=int(sum(v["n"] for v in pr.values())),
                                           panel_us_per_launch={q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in pr.items() if "given_panel" in q},
                                           rounds=int(pr.get("given_panel_stage", {}).get("n", 0)))
            out["profile"] = prof
            out["profile_overhead_us"] = ctx.profile_overhead_us()
            ctx.profile_enable(False)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "panel":
        panel(sys.argv[2] if len(sys.argv) > 2 else "large-v2")
        sys.exit(0)
    cost(sys.argv[1] if len(sys.argv) > 1 else "large-v2", int(sys.argv[2]) if len(sys.argv) > 2 else 56,
         int(sys.argv[3]) if len(sys.argv) > 3 else 64)
