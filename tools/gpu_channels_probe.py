"""Measurements of the multichannel front on one GPU: 56 x 30 s of stereo int16 at 48000 and at 44100 Hz,
per-family HIP-event time (Context.profile(); mean of 5 launches after a warm-up call; all buffers on the device):

    resample_mix, two identity rows            against   two resample calls on the pre-split channels
    resample_mix, two identity rows / one mean row   against   the one mean resample call
    channel_activity on the two-row output

    python tools/gpu_channels_probe.py
Prints one JSON line per rate."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402

b = pkg.binding
R, SECONDS, LAUNCHES = 56, 30, 5


def family_ms(ctx, name, per=1):
    v = ctx.profile()[name]
    assert v["n"] == LAUNCHES * per, (name, v)
    return v["ms"] / LAUNCHES


def timed(ctx, name, call, per=1):
    for it in range(LAUNCHES + 1):
        if it == 1:
            ctx.profile_reset()
        call()
    return family_ms(ctx, name, per)


def main():
    ctx = b.Context()
    ctx.profile_enable(True)
    lib, h, p = ctx.lib, ctx.handle, b._ptr
    rng = np.random.default_rng(0)
    for sr in (48000, 44100):
        n = SECONDS * sr
        stereo = [rng.integers(-20000, 20000, size=(n, 2), dtype=np.int64).astype(np.int16) for _ in range(R)]
        pcm, offs, ch, rates = b._pack_interleaved(stereo, [sr] * R)
        halves = [b._pack_interleaved([x[:, c].copy() for x in stereo], [sr] * R) for c in (0, 1)]
        n_out = b.resample_out_len(n, sr)
        d_pcm = ctx.to_device(pcm)
        d_half = [ctx.to_device(hv[0]) for hv in halves]
        d_out = ctx.dev_malloc(2 * R * n_out * 4)
        d_act = ctx.dev_malloc(2 * R * -(-n_out // 160) * 4)
        two, two_w = np.full(R, 2, np.int32), np.tile(np.eye(2, dtype=np.float32).reshape(-1), R)
        one, one_w = np.full(R, 1, np.int32), np.full(2 * R, 0.5, np.float32)
        sig_offs = (np.arange(2 * R + 1, dtype=np.int64) * n_out)

        def check(st):
            if st != 0:
                raise RuntimeError(lib.wm_last_error())

        def mix(rows, w):
            check(lib.wm_resample_16k_mix(h, d_pcm, 0, p(offs), p(ch), p(rates), R, p(rows), p(w), d_out, 1))

        def split_calls():
            for c in (0, 1):
                _, o1, c1, r1 = halves[c]
                check(lib.wm_resample_16k(h, d_half[c], 0, p(o1), p(c1), p(r1), R, d_out, 1))

        out = dict(rate=sr, recordings=R, seconds=SECONDS, in_MB=round(pcm.nbytes / 1e6, 1), signal_MB=round(R * n_out * 4 / 1e6, 1),
                   taps=int(-(-(2 * b.resample_filter(sr)[3] + 1) // b.resample_filter(sr)[1])) if sr != 16000 else 0)
        out["resample_mean_ms"] = timed(ctx, "resample", lambda: check(
            lib.wm_resample_16k(h, d_pcm, 0, p(offs), p(ch), p(rates), R, d_out, 1)))
        out["resample_two_mono_calls_ms"] = timed(ctx, "resample", split_calls, per=2)
        out["resample_mix_mean_row_ms"] = timed(ctx, "resample_mix", lambda: mix(one, one_w))
        out["resample_mix_two_rows_ms"] = timed(ctx, "resample_mix", lambda: mix(two, two_w))
        out["channel_activity_ms"] = timed(ctx, "channel_activity", lambda: check(
            lib.wm_channel_activity(h, d_out, p(sig_offs), 2 * R, d_act, 1)))
        out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}
        out["profile_overhead_us"] = round(ctx.profile_overhead_us(), 2)
        print(json.dumps(out), flush=True)
        for d in [d_pcm, d_out, d_act] + d_half:
            ctx.dev_free(d)
    ctx.close()


if __name__ == "__main__":
    main()
