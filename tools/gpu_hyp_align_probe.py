"""Cost of decode-pass word timestamps for beam-search and best-of hypotheses on ONE round of identical windows: synthetic lively
weights of the model given as argv[1] (default large-v2), 8 windows x 224 generated tokens behind [sot, language, task], early
stop off.  For beam_size = 5 and for best_of = 5 (temperature 0.7), interleaved in one process, four runs each after a warm-up:
`plain` (wm_transcribe_mel_beam / wm_transcribe_mel_best_of), `aligned` (the *_aligned entry: the same outputs asserted), and the
two-pass route `plain` + wm_align_mel over the chosen hypothesis' tokens < eot at teacher_panel 1 and 8.  Prints one JSON line:
wall seconds, the decode-loop time (wm_last_stage_ms[2]: for `aligned` with the gather, the alignment kernels and the DTW), and
from the per-family profile of one eager aligned call of each family the times of align_gather and of the tail.

    python tools/gpu_hyp_align_probe.py [model]"""
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
B, new, P, N = 8, 224, 3, 5
n = np.arange(480000, dtype=np.float64)
pcm = np.stack([(0.3 * np.sin(2 * np.pi * (200 + 370 * i) * n / 16000) * (0.5 + 0.5 * np.sin(2 * np.pi * (0.3 + 0.1 * i) * n / 16000))).astype(np.float32)
                for i in range(B)])
mel = ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32)
base = np.arange(B, dtype=np.int64) * (dims["n_mels"] * 3000)
prompts = np.array([[50258, 50259, 50359]] * B, dtype=np.int32)
EOT, NO_TS, NS = 50257, 50363, 50362
win = (mel, base, 3000, 0, 3000, prompts, new)
LABELS = ("plain", "aligned", "plain_align_panel1", "plain_align_panel8")


def decode(family, aligned):
    if family == "beam":
        fn = ctx.transcribe_mel_beam_aligned if aligned else ctx.transcribe_mel_beam
        return fn(*win, N, eot=-1, no_speech_token=NS)
    fn = ctx.transcribe_mel_best_of_aligned if aligned else ctx.transcribe_mel_best_of
    return fn(*win, N, eot=-1, temperature=0.7, seed=5, no_speech_token=NS)


out = dict(model=name, windows=B, new=new, rows_per_window=N, positions=P + new - 1,
           heads=dims["n_text_layer"] // 2 * dims["n_text_head"])
for family in ("beam", "best_of"):
    walls = {k: [] for k in LABELS}
    loops = {"plain": [], "aligned": []}
    for rep in range(5):
        for label in LABELS:
            t0 = time.perf_counter()
            r = decode(family, label == "aligned")
            ms = float(ctx.last_stage_ms()[2])
            if label.startswith("plain_align"):   # the two-pass route: the teacher-forced alignment of the hypothesis just chosen
                ctx.set_teacher_panel(int(label[-1]))
                sel = r.selected
                texts = [[int(t) for t in sel.tokens[i, :sel.lens[i]] if t < EOT] for i in range(B)]
                ctx.align_mel(mel, base, 3000, 0, 3000, texts, [50258, 50259, 50359], NO_TS, EOT)
            w = time.perf_counter() - t0
            if rep:   # the first of each is the warm-up (buffers, graphs)
                walls[label].append(w)
                if label in loops:
                    loops[label].append(ms)
            if label == "plain":
                want = r
            elif label == "aligned":
                assert np.array_equal(want.tokens, r.tokens) and np.array_equal(want.best, r.best)
                assert np.array_equal(want.logprobs.view(np.uint32), r.logprobs.view(np.uint32))
    ctx.set_teacher_panel(1)
    med = {k: float(np.median(v)) for k, v in walls.items()}
    # one profiled aligned call (eager launches): the families the feature adds
    ctx.profile_enable(True)
    ctx.profile_reset()
    decode(family, True)
    prof = ctx.profile()
    ctx.profile_enable(False)
    tail = {k: prof[k] for k in ("align_gather", "align_stats", "align_matrix", "align_dtw", "align_capture", "beam_select", "beam_reorder")
            if k in prof}
    out[family] = dict(wall_s=walls, median_wall_s=med, decode_loop_ms=loops, aligned_over_plain=med["aligned"] / med["plain"],
                       aligned_over_panel8=med["aligned"] / med["plain_align_panel8"], profile_aligned_call=tail)
print(json.dumps(out))
