"""Cost of the alignment from the decode's own pass on ONE round of identical windows (tools/gpu_longform_probe.py --words --decode
measures whole long-form runs, whose window count follows the word times): synthetic lively weights of the model given as
argv[1] (default large-v2), 8 windows x 224 generated tokens behind [sot, language, task], early stop off.  Interleaved, four runs
each after a warm-up: `plain` (wm_transcribe_mel), `aligned` (wm_transcribe_mel_aligned: asserted the same tokens), and the
two-pass route `plain` + wm_align_mel over the generated tokens < eot at teacher_panel 1 and 8.  Prints one JSON line: wall
seconds, the decode-loop time (wm_last_stage_ms[2]: for `aligned` with the alignment kernels and the DTW) per position, and the
per-family profile of one eager aligned call.

    python tools/gpu_decode_align_probe.py [model]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
name = sys.argv[1] if len(sys.argv) > 1 else "large-v2"
dims = dict(b.MODEL_DIMS[name])
ctx = b.Context(dims)
ctx.init_synthetic(3)
gain = W.lively_gain(dims)
for tname, shape, kind in W.tensor_specs(dims):
    if kind == W.K_MATRIX and "positional" not in tname:
        ctx.set_tensor(tname, ctx.get_tensor(tname, shape) * np.float32(gain))
ctx.finalize()
B, new, P = 8, 224, 3
n = np.arange(480000, dtype=np.float64)
pcm = np.stack([(0.3 * np.sin(2 * np.pi * (200 + 370 * i) * n / 16000) * (0.5 + 0.5 * np.sin(2 * np.pi * (0.3 + 0.1 * i) * n / 16000))).astype(np.float32)
                for i in range(B)])
mel = ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32)
base = np.arange(B, dtype=np.int64) * (dims["n_mels"] * 3000)
prompts = np.array([[50258, 50259, 50359]] * B, dtype=np.int32)
EOT, NO_TS = 50257, 50363
runs = {"plain": [], "aligned": []}
walls = {"plain": [], "aligned": [], "plain_align_panel1": [], "plain_align_panel8": []}
for rep in range(5):
    for label in ("plain", "aligned", "plain_align_panel1", "plain_align_panel8"):
        t0 = time.perf_counter()
        if label == "aligned":
            r = ctx.transcribe_mel_aligned(mel, base, 3000, 0, 3000, prompts, new, eot=-1, no_speech_token=50362)
        else:
            r = ctx.transcribe_mel(mel, base, 3000, 0, 3000, prompts, new, eot=-1, no_speech_token=50362)
        ms = float(ctx.last_stage_ms()[2])
        if label.startswith("plain_align"):   # the two-pass route: the teacher-forced alignment of the tokens just decoded
            ctx.set_teacher_panel(int(label[-1]))
            texts = [[int(t) for t in r.tokens[i] if t < EOT] for i in range(B)]
            ctx.align_mel(mel, base, 3000, 0, 3000, texts, [50258, 50259, 50359], NO_TS, EOT)
        w = time.perf_counter() - t0
        if rep:   # the first of each is the warm-up (buffers, graphs)
            walls[label].append(w)
            if label in runs:
                runs[label].append(ms)
        if label == "plain":
            tok = r.tokens
        elif label == "aligned":
            assert np.array_equal(tok, r.tokens)
ctx.set_teacher_panel(1)
pos = P + new - 1
med = {k: float(np.median(v)) for k, v in runs.items()}
out = dict(model=name, windows=B, new=new, positions=pos, heads=dims["n_text_layer"] // 2 * dims["n_text_head"], decode_loop_ms=runs,
           wall_s=walls, median_wall_s={k: float(np.median(v)) for k, v in walls.items()}, ms_per_position={k: v / pos for k, v in med.items()}, aligned_over_plain=med["aligned"] / med["plain"])
# one profiled aligned call (eager launches): the families the feature adds or reroutes
ctx.profile_enable(True)
ctx.profile_reset()
ctx.transcribe_mel_aligned(mel, base, 3000, 0, 3000, prompts, new, eot=-1, no_speech_token=50362)
prof = ctx.profile()
ctx.profile_enable(False)
out["profile_aligned_call"] = prof
print(json.dumps(out))
