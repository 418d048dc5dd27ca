"""Cost of wm_align at large-v2 (synthetic weights, full depth): 8 chunks x 224 text tokens, default alignment heads
(every head of decoder layers 16 .. 31 = 320 heads), sot sequence of 3 tokens.  Prints the wall time of the call and its
stage split (wm_last_stage_ms: front end + encoder + cross K/V, teacher-forced pass, alignment kernels + DTW)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402

B, N_TEXT, REPS = 8, 224, 3
dims = pkg.binding.MODEL_DIMS["large-v2"]
ctx = pkg.binding.Context(dims)
ctx.init_synthetic(1)
ctx.finalize()
rng = np.random.default_rng(0)
n = np.arange(480000) / 16000.0
pcm = np.stack([(0.3 * np.sin(2 * np.pi * (200 + 90 * i) * n)).astype(np.float32) for i in range(B)])
texts = [[int(t) for t in rng.integers(0, 50257, size=N_TEXT)] for _ in range(B)]
ctx.align(pcm, texts, [50258, 50259, 50359], 50363, 50257)   # warm-up
walls, stages = [], []
for _ in range(REPS):
    t0 = time.perf_counter()
    ctx.align(pcm, texts, [50258, 50259, 50359], 50363, 50257)
    walls.append(time.perf_counter() - t0)
    stages.append(ctx.last_stage_ms().tolist())
st = np.median(np.array(stages), axis=0)
res = dict(model="large-v2", chunks=B, text_tokens=N_TEXT, heads=320, wall_s=sorted(walls),
           stage_ms=dict(frontend_encoder=float(st[0]), teacher_forced=float(st[1]), alignment=float(st[2])),
           teacher_forced_ms_per_position=float(st[1]) / (3 + N_TEXT + 2),
           alignment_share_of_teacher_forced=float(st[2] / st[1]))
print(json.dumps(res))
