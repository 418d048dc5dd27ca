"""Cost of wm_align at large-v2 (synthetic weights, full depth): 8 chunks x 224 text tokens, default alignment heads
(every head of decoder layers 16 .. 31 = 320 heads), sot sequence of 3 tokens.  Prints the wall time of the call and its
stage split (wm_last_stage_ms: front end + encoder + cross K/V, teacher-forced pass, alignment kernels + DTW).

    --teacher-panel W[,W...]  one result line per panel width (wm_set_teacher_panel); without it no setter call is made
                              (the library's default, width 1 -- also what a library from before the option runs)
    --chunks B                chunks of the call (default 8; more than 16 exercises the slices of a panel pass)
    --model NAME              binding.MODEL_DIMS key (default large-v2)
    --cut narrow|slices       (debug library) force one of the two candidate cuts of a group of more windows than fit a full-width
                              panel: ONE panel narrowed to floor(128 / chunks) positions, or slices of 128 / W windows at width W
                              (without it: the library's rule, the cut with the fewest steps)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--teacher-panel", default=None)
ap.add_argument("--chunks", type=int, default=8)
ap.add_argument("--model", default="large-v2")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cut", choices=("narrow", "slices"), default=None)
args = ap.parse_args()

B, N_TEXT, REPS = args.chunks, 224, args.reps
dims = pkg.binding.MODEL_DIMS[args.model]
ctx = pkg.binding.Context(dims, debug=args.cut is not None)
if args.cut:
    import ctypes
    ctx.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    assert ctx.lib.wmdbg_set_tuning(b"teacher_panel_cut", 1 if args.cut == "narrow" else 2) == 0
ctx.init_synthetic(1)
ctx.finalize()
rng = np.random.default_rng(0)
n = np.arange(480000) / 16000.0
pcm = np.stack([(0.3 * np.sin(2 * np.pi * (200 + 90 * (i % 8)) * n)).astype(np.float32) for i in range(B)])
texts = [[int(t) for t in rng.integers(0, 50257, size=N_TEXT)] for _ in range(B)]
L, H = dims["n_text_layer"], dims["n_text_head"]
first = None
for width in ([None] if args.teacher_panel is None else [int(w) for w in args.teacher_panel.split(",")]):
    if width is not None:
        ctx.set_teacher_panel(width)
    out = ctx.align(pcm, texts, [50258, 50259, 50359], 50363, 50257)   # warm-up
    if first is None:
        first = out
    same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(out, first))
    walls, stages = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        ctx.align(pcm, texts, [50258, 50259, 50359], 50363, 50257)
        walls.append(time.perf_counter() - t0)
        stages.append(ctx.last_stage_ms().tolist())
    st = np.median(np.array(stages), axis=0)
    res = dict(model=args.model, chunks=B, text_tokens=N_TEXT, heads=(L - L // 2) * H, teacher_panel=width, cut=args.cut or "rule", wall_s=sorted(walls),
               stage_ms=dict(frontend_encoder=float(st[0]), teacher_forced=float(st[1]), alignment=float(st[2])),
               teacher_forced_ms_runs=[float(s[1]) for s in stages],
               teacher_forced_ms_per_position=float(st[1]) / (3 + N_TEXT + 2),
               alignment_share_of_teacher_forced=float(st[2] / st[1]), same_bits_as_first_width=bool(same))
    print(json.dumps(res), flush=True)
