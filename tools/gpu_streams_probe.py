"""Live streams against the only way to do the same without them (DESIGN.md "Live streams").

    python tools/gpu_streams_probe.py [S]

S = 64 streams (int16, 16 kHz), each holding 30 s of audio, get one packet each per update -- 20 ms, 100 ms and 1 s packets --
and the last 3000 frames of every stream are wanted as a normalised block on the device after every update:

    streams : Streams.push of the S packets (host memory) + wm_streams_window of S rows of 3000 frames (device memory);
    long    : the S streams' last 30 s of samples, kept packed on the host, uploaded, and wm_logmel_long over all of them
              (6000 frames per stream: the 480000 zeros that follow a recording are part of that entry).

Each figure is a host clock around calls that end in a device synchronise, per update, over a third of a second or so of
updates after a warm-up of both sides; the two sides alternate, three rounds each, and every round is printed (the spread is
the noise).  The device buffers of both sides are allocated once.  A second pass reports the HIP-event time of
the kernel families alone.  Prints JSON lines."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402

b = pkg.binding
PACKETS = ((320, 3000), (1600, 2400), (16000, 1500))   # (samples per packet, timed updates: a third of them per round)
N_LONG = 100                                            # timed updates of the other side per round


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    ctx = b.Context()
    rng = np.random.default_rng(0)
    t = np.arange(480000 + 16000 * 40) / 16000.0
    audio = [np.clip(np.round(32768 * (0.3 * np.sin(2 * np.pi * (150 + 13 * s) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.3 * t))
                                       + 0.01 * rng.standard_normal(t.size))), -32768, 32767).astype(np.int16) for s in range(S)]
    print(json.dumps(dict(S=S, dtype="int16", window_frames=3000, prefill_s=30)))
    for packet, iters in PACKETS:
        st = b.Streams(ctx, S, capacity_frames=3003 + packet // 160 + 4)
        st.push([a[:480000] for a in audio])
        at = [480000]
        rows = np.arange(S, dtype=np.int32)
        n3000 = np.full(S, 3000, np.int32)
        win_base = np.arange(S, dtype=np.int64) * 80 * 3000
        # the device buffers of both sides are allocated once: an update is copies and launches alone
        d_win = ctx.dev_malloc(S * 80 * 3000 * 4)
        d_pcm = ctx.dev_malloc(S * 480000 * 2)
        d_long = ctx.dev_malloc(S * 80 * 6000 * 4)

        def update_streams():
            st.push([a[at[0]:at[0] + packet] for a in audio])
            at[0] = 480000 + (at[0] - 480000 + packet) % (16000 * 39)   # (what the packets hold plays no part in the time)
            A = st.frames()[2]
            first = np.ascontiguousarray(A - 3000)
            b._check(ctx.lib, ctx.lib.wm_streams_window(ctx.handle, st.handle, S, b._ptr(rows), b._ptr(first), b._ptr(n3000), d_win,
                                                        b._ptr(win_base), b.WM_MEM_DEVICE))   # (synchronises)

        packed = np.concatenate([a[:480000] for a in audio])
        offs = (np.arange(S + 1, dtype=np.int64) * 480000)

        def update_long():
            ctx.upload(d_pcm, packed)
            b._check(ctx.lib, ctx.lib.wm_logmel_long(ctx.handle, d_pcm, b.WM_I16, b._ptr(offs), S, 80, d_long,
                                                     b.WM_MEM_DEVICE))   # (synchronises)

        n_long = N_LONG
        for _ in range(3):
            update_streams()
            update_long()
        rounds = dict(streams_ms=[], long_ms=[])
        for r in range(3):
            k = iters // 3
            t0 = time.perf_counter()
            for _ in range(k):
                update_streams()
            rounds["streams_ms"].append((time.perf_counter() - t0) / k * 1e3)
            t0 = time.perf_counter()
            for _ in range(n_long):
                update_long()
            rounds["long_ms"].append((time.perf_counter() - t0) / n_long * 1e3)
        # kernel families alone (HIP events), a pass of its own
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(10):
            update_streams()
        for _ in range(3):
            update_long()
        prof = ctx.profile()
        ctx.profile_enable(False)
        fam = {k: round(v["ms"] / v["n"] * 1e3, 2) for k, v in prof.items() if isinstance(v, dict) and v.get("n")}
        new_frames = packet // 160 + 3
        print(json.dumps(dict(packet_samples=packet, packet_ms=packet / 16.0, updates_per_round=iters // 3, long_per_round=n_long,
                              streams_ms_per_update=[round(v, 3) for v in rounds["streams_ms"]],
                              long_ms_per_update=[round(v, 3) for v in rounds["long_ms"]],
                              kernel_us_per_launch=fam, frames_computed_per_stream=new_frames,
                              workgroup_frames=64, workgroup_fill=round(new_frames / (64.0 * ((new_frames + 63) // 64)), 3),
                              upload_bytes_streams=S * packet * 2, upload_bytes_long=int(packed.nbytes))))
        st.close()
        for d in (d_win, d_pcm, d_long):
            ctx.dev_free(d)
    ctx.close()


if __name__ == "__main__":
    main()
