"""Throughput of long-form transcription (binding.transcribe_long: whole-recording log-mel, seek-based windows decoded in
lockstep across recordings, temperature fallback) against the fixed 30 s windows of wm_transcribe over the same audio
(every recording cut at multiples of 480000 samples, the last piece zero-padded).  Synthetic weights of the multilingual model
given as argv[1] (default base), every matrix scaled by weights.lively_gain so that the decode depends on the audio, N recordings of mixed
length (argv[2], default 8: 10 .. 150 s), the production vocabulary's token ids, text context n_text_ctx.  Prints one JSON
line: wall seconds and audio-s/s of both, windows decoded and fallback steps taken by the long form."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
name = sys.argv[1] if len(sys.argv) > 1 else "base"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dims = dict(b.MODEL_DIMS[name])
SOT, TASK, NS, TSB, EOT = 50258, 50359, 50362, 50364, 50257
ctx = b.Context(dims)
ctx.init_synthetic(3)
gain = W.lively_gain(dims)
for tname, shape, kind in W.tensor_specs(dims):
    if kind == W.K_MATRIX and "positional" not in tname:
        ctx.set_tensor(tname, ctx.get_tensor(tname, shape) * np.float32(gain))
ctx.finalize()
ctx.set_suppress([SOT, 50358, 50361, NS, 50363], [220, EOT])
rng = np.random.default_rng(0)
recs = []
for i in range(N):
    n = int(rng.integers(10, 151)) * 16000 + int(rng.integers(0, 16000))
    t = np.arange(n) / 16000.0
    recs.append((0.3 * np.sin(2 * np.pi * (180 + 60 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.2 * t))).astype(np.float32))
audio_s = sum(r.size for r in recs) / 16000.0
kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, language=50259)
ctx.transcribe_long(recs[:1], **kw)    # warm-up: graphs, buffers
t0 = time.perf_counter()
out = ctx.transcribe_long(recs, **kw)
wall_long = time.perf_counter() - t0
windows = sum(len(o["windows"]) for o in out)
steps = sum(len(w["temperatures"]) for o in out for w in o["windows"])
# fixed 30 s windows of the same audio, one wm_transcribe call, the same prompt and sample length
chunks = []
for r in recs:
    for s in range(0, r.size, 480000):
        c = np.zeros(480000, np.float32)
        piece = r[s:s + 480000]
        c[:piece.size] = piece
        chunks.append(c)
pcm = np.stack(chunks)
max_new = dims["n_text_ctx"] // 2
ctx.set_timestamp_rules(True, TSB, EOT, 50)
ctx.transcribe(pcm[:1], [SOT, 50259, TASK], max_new, eot=EOT, no_speech_token=NS)
t0 = time.perf_counter()
ctx.transcribe(pcm, [SOT, 50259, TASK], max_new, eot=EOT, no_speech_token=NS)
wall_fixed = time.perf_counter() - t0
print(json.dumps(dict(model=name, recordings=N, audio_s=audio_s, long_wall_s=wall_long,
                      long_audio_s_per_s=audio_s / wall_long, long_windows=windows, long_decode_steps=steps,
                      fixed_chunks=len(chunks), fixed_wall_s=wall_fixed, fixed_audio_s_per_s=audio_s / wall_fixed)))
