"""Two measurements of the speech-activity path.

    python tools/gpu_vad_probe.py kernel
        wm_vad_energy next to wm_logmel_long on the recordings of tools/gpu_longform_probe.py (8 recordings of 10 .. 150 s):
        per-family HIP-event time (mean of 5 launches after a warm-up), the band's bytes and bytes/s.

    python tools/gpu_vad_probe.py clips [model]
        One 10-minute recording of tone bursts over faint noise, synthetic lively weights of `model` (default base),
        temperatures=(0.0,): wall time of the sequential clip run (transcribe_long(clip_timestamps=...), the path that
        existed before parallel_clips) against parallel_clips=56 on the same clips, interleaved, three runs each after a
        warm-up of each, with the rounds (decode calls) and windows of a run.  The two results are asserted equal.
Prints JSON lines."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
SOT, TASK, NS, TSB, EOT = 50258, 50359, 50362, 50364, 50257


def kernel():
    ctx = b.Context()
    rng = np.random.default_rng(0)
    recs = []
    for i in range(8):
        n = int(rng.integers(10, 151)) * 16000 + int(rng.integers(0, 16000))
        t = np.arange(n) / 16000.0
        recs.append((0.3 * np.sin(2 * np.pi * (180 + 60 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.2 * t))).astype(np.float32))
    pcm, offs = b._pack_recordings(recs)
    d_pcm = ctx.to_device(pcm)
    lo, hi = b.vad_band(80)
    ctx.profile_enable(True)
    out = {}
    for label, band in (("speech band", (lo, hi)), ("all 80 bins", (0, 80))):
        for it in range(6):
            if it == 1:
                ctx.profile_reset()
            d_mel, mel_offs, T = ctx.logmel_long_device(d_pcm, np.float32, offs)
            content = T - 3000
            ctx.vad_energy(d_mel, mel_offs[:8], T, content, band, 5, device=True)
            ctx.dev_free(d_mel)
        prof = ctx.profile()
        fam = {k: v["ms"] / v["n"] for k, v in prof.items() if isinstance(v, dict) and v.get("n")} if isinstance(prof, dict) else prof
        nbytes = (band[1] - band[0]) * int(content.sum()) * 4
        out[label] = dict(families_ms=fam, frames=int(content.sum()), band_bytes=nbytes,
                          vad_GBps=nbytes / (fam["vad"] * 1e-3) / 1e9 if isinstance(fam, dict) and "vad" in fam else None)
    out["audio_s"] = sum(r.size for r in recs) / 16000.0
    out["profile_overhead_us"] = ctx.profile_overhead_us()
    print(json.dumps(dict(kernel=out)))


def clips(name):
    dims = dict(b.MODEL_DIMS[name])
    ctx = b.Context(dims)
    ctx.init_synthetic(3)
    gain = W.lively_gain(dims)
    for tname, shape, kind in W.tensor_specs(dims):
        if kind == W.K_MATRIX and "positional" not in tname:
            ctx.set_tensor(tname, ctx.get_tensor(tname, shape) * np.float32(gain))
    ctx.finalize()
    ctx.set_suppress([SOT, 50358, 50361, NS, 50363], [220, EOT])
    rng = np.random.default_rng(1)
    n = 600 * 16000
    t = np.arange(n) / 16000.0
    x = 0.0005 * rng.standard_normal(n)
    tone = 0.3 * np.sin(2 * np.pi * 310 * t) * (0.75 + 0.25 * np.sin(2 * np.pi * 3.0 * t))
    at, spans = 1.0, []
    while at < 590.0:   # bursts of 2 .. 14 s, pauses of 1 .. 4 s
        d = float(rng.uniform(2.0, 14.0))
        z = min(at + d, 598.0)
        spans.append((at, z))
        x[int(at * 16000):int(z * 16000)] += tone[int(at * 16000):int(z * 16000)]
        at = z + float(rng.uniform(1.0, 4.0))
    rec = x.astype(np.float32)
    kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, language=50259, temperatures=(0.0,))
    found = ctx.transcribe_long([rec], vad=True, **kw)[0]
    times = [[v / 100.0 for ab in found["vad_clips"] for v in ab]]
    calls = []
    inner = ctx.transcribe_mel

    def counted(*a, **k):
        calls.append(len(a[3]))
        return inner(*a, **k)
    ctx.transcribe_mel = counted
    runs = dict(sequential=dict(clip_timestamps=times), parallel=dict(clip_timestamps=times, parallel_clips=56))
    res = {k: dict(wall_s=[]) for k in runs}
    outs = {}
    for k, extra in runs.items():
        ctx.transcribe_long([rec], **kw, **extra)   # warm-up
    for _ in range(3):
        for k, extra in runs.items():
            del calls[:]
            t0 = time.perf_counter()
            outs[k] = ctx.transcribe_long([rec], **kw, **extra)[0]
            res[k]["wall_s"].append(round(time.perf_counter() - t0, 4))
            res[k].update(rounds=len(calls), windows=len(outs[k]["windows"]), rows_per_round_max=max(calls))
    strip = lambda o: dict(o, windows=[{q: v for q, v in w.items() if q != "round"} for w in o["windows"]])  # noqa: E731
    assert strip(outs["parallel"]) == outs["sequential"]
    for k in res:
        res[k]["audio_s_per_s"] = round(600.0 / min(res[k]["wall_s"]), 1)
    print(json.dumps(dict(model=name, bursts=len(spans), speech_s=round(sum(z - a for a, z in spans), 1),
                          vad_segments=len(found["vad_segments"]), vad_clips=len(found["vad_clips"]), runs=res,
                          speedup=round(min(res["sequential"]["wall_s"]) / min(res["parallel"]["wall_s"]), 2),
                          rounds_ratio=round(res["sequential"]["rounds"] / res["parallel"]["rounds"], 2))))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "clips":
        clips(sys.argv[2] if len(sys.argv) > 2 else "base")
    else:
        kernel()
