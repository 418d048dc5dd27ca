"""GPU probe: cost of wm_transcribe's extended decode (log-probs, sampling) against wm_transcribe_greedy, in ms per decode
position, as interleaved A/B runs on one device: greedy | log-probs at T = 0 | sampling at T = 1 (log-probs + no-speech).

    python tools/gpu_transcribe_options_probe.py [reps] [model:batch,...] [modes]   (default: 5, large-v2:56,tiny.en:1, all)

modes: a comma list of greedy / logprobs / sample (one mode per process is what a rocprofv3 --kernel-trace --stats run of
each wants: profiles/r07_transcribe_options_kernels.txt).

One decode group per call (wm_set_lanes(1)), fixed length (eot = -1); the decode stage time is wm_last_stage_ms()[2]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402

B = pkg.binding


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cfgs = (("large-v2", 56), ("tiny.en", 1))
    if len(sys.argv) > 2:
        cfgs = tuple((m, int(b)) for m, b in (c.split(":") for c in sys.argv[2].split(",")))
    new = 96
    print("ms per decode position (median of %d interleaved runs; min in brackets), %d new tokens" % (reps, new))
    for model, nb in cfgs:
        dims = B.MODEL_DIMS[model]
        ctx = B.Context(dims)
        ctx.init_synthetic(20240928, matrix_gain=4.0)
        ctx.finalize()
        ctx.set_lanes(1)
        rng = np.random.default_rng(1)
        pcm = np.round(np.clip(0.1 * rng.standard_normal((nb, 480000)), -1, 1) * 32767).astype(np.int16)
        multi = dims["n_vocab"] >= 51865
        prompt = [50258, 50259, 50359, 50363] if multi else [50257, 50362]
        ns_tok = 50362 if multi else 50361
        n_pos = len(prompt) + new - 1
        modes = {
            "greedy": lambda: ctx.transcribe_greedy(pcm, prompt, new, eot=-1)[0],
            "logprobs T=0": lambda: ctx.transcribe(pcm, prompt, new, temperature=0.0).tokens,
            "sample T=1": lambda: ctx.transcribe(pcm, prompt, new, temperature=1.0, seed=3, no_speech_token=ns_tok).tokens,
        }
        if len(sys.argv) > 3:
            keep = sys.argv[3].split(",")
            modes = {k: f for k, f in modes.items() if k.split()[0] in keep}
        times = {k: [] for k in modes}
        toks = {}
        for k, f in modes.items():   # warm-up: graph captures
            toks[k] = f()
        for _ in range(reps):
            for k, f in modes.items():
                f()
                times[k].append(float(ctx.last_stage_ms()[2]) / n_pos)
        g = float(np.median(times["greedy"])) if "greedy" in times else float("nan")
        same = np.array_equal(toks["greedy"], toks["logprobs T=0"]) if len(modes) == 3 else "n/a"
        row = []
        for k in modes:
            m = float(np.median(times[k]))
            row.append("%s %.4f [%.4f] (%+.1f %%)" % (k, m, min(times[k]), 100.0 * (m / g - 1.0)))
        print("%-9s B=%-3d %s  | T=0 tokens == greedy: %s" % (model, nb, " | ".join(row), same), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
