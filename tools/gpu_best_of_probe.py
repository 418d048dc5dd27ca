"""Cost of best-of-N sampling: wm_transcribe_mel_best_of (the N candidates of a window share its encoder pass, its cross-K/V
cache and every read of it) against the only way a build without it has -- wm_transcribe_mel with every window passed N
times under N sample ids.  Synthetic lively weights of the model given as argv[1] (default large-v2), temperature 1,
eot = -1 (fixed length), 224 new tokens, best_of 5 (--best-of N), at 8 and at 24 windows (--windows 8,24).

    python tools/gpu_best_of_probe.py [model] [--mode best_of | replicate] [--runs 3] [--new 224] [--windows 8,24]

--mode best_of   : the new call (needs a build that has it);
--mode replicate : N x B rows through wm_transcribe_mel, row b * N + s = window b under sample id s << 16 | b -- works on a
                   build of the parent commit too, which is what it is for: run the two builds alternately on one box.
Prints one JSON line per (windows, run): wall seconds, wm_last_stage_ms (front end / encoder + cross K/V / decode), and the
per-position time (decode stage over the positions stepped).  The cross-attention launch time comes from a run of its own,
eager (graph replays are not traceable) and on one lane, so that the 24-window call is one group of 120 rows:
`WM_NO_GRAPH=1 WM_LANES=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rp -- python
tools/gpu_best_of_probe.py large-v2 --mode MODE --runs 1 --windows 24`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


mode = _opt("--mode", "best_of")
runs = int(_opt("--runs", "3"))
NEW = int(_opt("--new", "224"))
N = int(_opt("--best-of", "5"))
windows = [int(x) for x in _opt("--windows", "8,24").split(",")]
name = sys.argv[1] if len(sys.argv) > 1 else "large-v2"
dims = dict(b.MODEL_DIMS[name])
SOT, TASK = 50258, 50359
PROMPT = [SOT, 50259, TASK]

ctx = b.Context(dims)
ctx.init_synthetic(3, matrix_gain=W.lively_gain(dims))
ctx.finalize()
n_mels = dims["n_mels"]
rng = np.random.default_rng(0)
pcm = np.zeros((max(windows), 480000), np.float32)
t = np.arange(480000) / 16000.0
for i in range(pcm.shape[0]):
    pcm[i] = 0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (0.2 + 0.05 * i) * t))
mel = ctx.logmel(pcm, n_mels=n_mels, out_dtype=np.float32)
d_mel = ctx.to_device(mel)
positions = len(PROMPT) + NEW - 1


def run(B):
    base = np.arange(B, dtype=np.int64) * (n_mels * 3000)
    prompts = np.tile(np.array(PROMPT, np.int32), (B, 1))
    ids = np.arange(B, dtype=np.uint32)
    t0 = time.perf_counter()
    if mode == "best_of":
        r = ctx.transcribe_mel_best_of(d_mel, base, 3000, 0, 3000, prompts, NEW, N, eot=-1, temperature=1.0, seed=11,
                                       sample_ids=ids, mem=b.WM_MEM_DEVICE)
        toks = r.tokens
    else:
        rep = np.repeat(np.arange(B), N)
        rid = (np.tile(np.arange(N, dtype=np.uint32), B) << np.uint32(16)) | ids[rep]
        r = ctx.transcribe_mel(d_mel, base[rep], 3000, 0, 3000, prompts[rep], NEW, eot=-1, temperature=1.0, seed=11,
                               sample_ids=rid, mem=b.WM_MEM_DEVICE)
        toks = r.tokens.reshape(B, N, NEW)
    wall = time.perf_counter() - t0
    st = [float(x) for x in ctx.last_stage_ms()]
    distinct = int(np.mean([len({tuple(c) for c in toks[w]}) for w in range(B)]) * 100) / 100.0
    return dict(model=name, mode=mode, windows=B, best_of=N, new=NEW, wall_s=round(wall, 4),
                stage_ms=[round(x, 3) for x in st], per_position_ms=round(st[2] / positions, 4),
                distinct_candidates_per_window=distinct)


try:
    for B in windows:
        run(B)   # warm-up: buffers, lanes, the position graphs
        for k in range(runs):
            print(json.dumps(dict(run(B), run=k)), flush=True)
finally:
    ctx.dev_free(d_mel)
    ctx.close()
