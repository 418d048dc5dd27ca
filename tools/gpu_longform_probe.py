"""Throughput of long-form transcription (binding.transcribe_long: whole-recording log-mel, seek-based windows decoded in
lockstep across recordings, temperature fallback) against the fixed 30 s windows of wm_transcribe over the same audio
(every recording cut at multiples of 480000 samples, the last piece zero-padded).  Synthetic weights of the multilingual model
given as argv[1] (default base), every matrix scaled by weights.lively_gain so that the decode depends on the audio, N recordings of mixed
length (argv[2], default 8: 10 .. 150 s), the production vocabulary's token ids, text context n_text_ctx.  Prints one JSON
line: wall seconds and audio-s/s of both, windows decoded and fallback steps taken by the long form.

    python tools/gpu_longform_probe.py [model] [recordings] [--condition | --prompt-panel W | --words [--teacher-panel W] [--decode] | --reuse
                                                            | --fallback {lockstep,deferred} [--fallback-share S] | --rows-position]

--condition: the cost of condition_on_previous_text instead.  One more JSON line: wall seconds of the long form with
conditioning off and on (the same recordings, after a warm-up of each; with the default fallback thresholds and with the
log-prob and compression-ratio thresholds off, where no window falls back and the prompts accumulate), the prompt positions and generated positions each
run decoded (per wm_transcribe_mel[_ragged] call: rows x the longest prompt of the call, rows x the longest generated
length), the position graphs captured (distinct (rows, prompt positions) pairs among the calls, against the 4 graph sets a
lane keeps), and the per-position time of ONE ragged decode group against a uniform group of the same size and the same
number of prompt positions (what the row-offset load in the self-attention launch costs).

--prompt-panel W: what wm_set_prompt_panel(W) is worth on --condition's conditioned run without fallback (the run whose prompts
accumulate).  ONE width per process, so that widths are compared in interleaved processes: after a warm-up, the wall seconds
of the run at that width (W = 1: the setter is not called at all, so the same line can be taken with another build's library,
WM_LIB_PATH), its calls, prompt steps and prompt positions, and from the plan (wmdbg_prompt_panel_plan, host only) the panel
steps that replaced them and the ordinary prompt steps left; then ONE uniform group of `recordings` rows with n_text_ctx / 2 + 3
prompt positions and a single new token, best of 4: the decode stage at width 1 and at W, and from the two the time per
ordinary prompt step and per panel step.  One JSON line.

--words: the cost of word_timestamps instead.  Fallback and the silence skip are off, so every window is kept and goes
through the alignment; a synthetic vocabulary (one piece per text token) is written to a temporary file.  One more JSON
line: wall seconds of the long form with word_timestamps off and on, interleaved, three runs each after a warm-up of
each, the windows and words of a run, and over the wm_align_mel calls of one run their number, rows, wall time and the
wm_last_stage_ms split (window gather + encoder + cross K/V, teacher-forced pass, alignment kernels + DTW).
--teacher-panel W (with --words): a third interleaved run, word_timestamps on with wm_set_teacher_panel(W) (label on_panel; the
plain `on` run is width 1); its result is asserted equal to the width-1 run's, and the line gains the panel run's stage split.
--decode (with --words): one more interleaved run, word_timestamps="decode" (label decode: the alignment from the decode's own
pass, no wm_align_mel call); the line gains its wall time over `off` and over the teacher-forced runs, whether its windows'
tokens are the `off` run's (the word-driven seek may cut other windows), and the decode-loop time (wm_last_stage_ms[2], the
alignment tail included) of its calls.

--reuse: the cost and the gain of reuse_encoder (window sets) instead.  Two configurations -- (a) the default fallback, where
the synthetic model takes all six temperatures, (b) fallback off with word_timestamps -- each with reuse_encoder off / on
interleaved, three runs each after a warm-up of each; the two runs' results are asserted equal.  One JSON line per
configuration: wall seconds, the wm_last_stage_ms splits summed over the calls of one run (off: staging, encoder + cross
K/V, decode of every wm_transcribe_mel call and the encoder part of every wm_align_mel call; on: the wm_windows_encode
calls and, per reading call, the copy from the set), the copy in GB/s (bytes read + bytes written) and per window next to
the encoder + cross-K/V cost per window of the off run.

--fallback {lockstep,deferred}: the temperature-fallback loop instead.  The synthetic model fails the
log-prob test on EVERY window, so --fallback-share S (default 1.0: the default thresholds, every window runs all six
temperatures) makes only a share fall back: a calibration run at temperature 0 without thresholds gives every window's
avg_logprob, and logprob_threshold is their S-quantile (the compression-ratio test is off).  The share is a stand-in for a real
checkpoint's, which nobody has measured here.  lockstep: three runs after a warm-up.  deferred: lockstep and deferred alternating,
three runs each after a warm-up of each, their results asserted equal (round numbers aside).  One JSON line: per variant the
wall seconds of every run, rounds (counted in the loop), decode calls, decode positions stepped (per call: its prompt positions + its longest generated
row) and rows x positions, plus the windows and the share that fell back.

--rows-position: the cost of one X-mode decode position with a sampling row map against without one (wm_set_sampling_rows), ONE
uniform group of `recordings` rows, 64 new tokens, eot off, alternating, best of 4: a sampling call at temperature 0.8, the same
call under a map of that pair for every row, under a map of mixed temperatures (0, 0.8, 0, 1.0 ...), and the three again with the
sampling rules (50, 0.9, 0) on.  One JSON line: ms per position (wm_last_stage_ms[2] / positions), and from one profiled call per
variant (eager launches, a HIP event pair round every launch) the mean us of the logits launch and of the truncation launch."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openai_whisper_coreml_amd as pkg  # noqa: E402
from openai_whisper_coreml_amd import weights as W  # noqa: E402

b = pkg.binding
CONDITION = "--condition" in sys.argv
WORDS = "--words" in sys.argv
REUSE = "--reuse" in sys.argv
DECODE = "--decode" in sys.argv
PPANEL = None
if "--prompt-panel" in sys.argv:
    i = sys.argv.index("--prompt-panel")
    PPANEL = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
PANEL = None
if "--teacher-panel" in sys.argv:
    i = sys.argv.index("--teacher-panel")
    PANEL = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
FALLBACK = None
if "--fallback" in sys.argv:
    i = sys.argv.index("--fallback")
    FALLBACK = sys.argv[i + 1]
    if FALLBACK not in ("lockstep", "deferred"):
        sys.exit("--fallback: lockstep or deferred")
    del sys.argv[i:i + 2]
SHARE = 1.0
if "--fallback-share" in sys.argv:
    i = sys.argv.index("--fallback-share")
    SHARE = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
ROWS_POSITION = "--rows-position" in sys.argv
argv = [a for a in sys.argv[1:] if a not in ("--condition", "--words", "--reuse", "--decode", "--rows-position")]
name = argv[0] if len(argv) > 0 else "base"
N = int(argv[1]) if len(argv) > 1 else 8
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


def condition_probe():
    SOT_PREV = 50361
    calls = []
    inner = ctx.transcribe_mel

    def counted(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k):
        t0 = time.perf_counter()
        r = inner(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k)
        calls.append(dict(rows=len(prompts), P=max(len(p) for p in prompts), gen=int(r.lens.max()),
                          wall=time.perf_counter() - t0))
        return r
    ctx.transcribe_mel = counted
    res = {}
    # the synthetic model fails the log-prob test on every window, so with the default thresholds every window ends at
    # temperature 1.0 and resets its recording's prompt: the runs without thresholds are the ones whose prompts accumulate
    cond = dict(condition_on_previous_text=True, sot_prev=SOT_PREV)
    nofb = dict(logprob_threshold=None, compression_ratio_threshold=None)
    for label, extra in (("off", {}), ("on", cond), ("off_no_fallback", nofb), ("on_no_fallback", dict(cond, **nofb))):
        ctx.transcribe_long(recs, **kw, **extra)     # warm-up: buffers, and whatever graphs survive
        del calls[:]
        t0 = time.perf_counter()
        out = ctx.transcribe_long(recs, **kw, **extra)
        wall = time.perf_counter() - t0
        shapes = [(c["rows"], c["P"]) for c in calls]
        recaptured, held = 0, []
        for sh in shapes:   # the LRU of 4 graph sets a lane keeps, replayed over the run's calls
            if sh in held:
                held.remove(sh)
            else:
                recaptured += 1
                if len(held) == 4:
                    held.pop(0)
            held.append(sh)
        res[label] = dict(wall_s=wall, audio_s_per_s=audio_s / wall, calls=len(calls),
                          windows=sum(len(o["windows"]) for o in out),
                          prompt_positions=sum(c["rows"] * c["P"] for c in calls),
                          generated_positions=sum(c["rows"] * c["gen"] for c in calls),
                          prompt_steps=sum(c["P"] for c in calls), generated_steps=sum(c["gen"] for c in calls),
                          distinct_graph_shapes=len(set(shapes)), graph_captures=recaptured,
                          first_call_of_a_shape_mean_s=float(np.mean([c["wall"] for i, c in enumerate(calls)
                                                                      if shapes.index(shapes[i]) == i])),
                          repeated_shape_mean_s=float(np.mean([c["wall"] for i, c in enumerate(calls)
                                                               if shapes.index(shapes[i]) != i] or [0.0])))
    ctx.transcribe_mel = inner
    # one ragged group against one uniform group: same rows, same prompt positions, fixed length (eot off)
    n_ctx = dims["n_text_ctx"]
    P, new = n_ctx // 2 + 3, 64
    d_mel, offs, T = ctx.logmel_long(recs, n_mels=dims["n_mels"], device=True)
    rows = list(range(N))
    prng = np.random.default_rng(5)
    uniform = [[int(t) for t in prng.integers(0, 50000, size=P - 3)] + [SOT, 50259, TASK] for _ in rows]
    lens = [P] + [3 + (P - 3) * i // N for i in range(1, N)]     # the longest first, then 3 + ... spread up to P
    ragged = [p[P - n:] for p, n in zip(uniform, lens)]
    per_pos = {}
    try:
        for label, prompts in (("uniform", uniform), ("ragged", ragged)):
            best = None
            for _ in range(4):
                ctx.transcribe_mel(d_mel, offs[rows], T[rows], 0, [min(3000, int(t) - 3000) for t in T[rows]], prompts, new,
                                   eot=-1, no_speech_token=NS, sot_tail=3, mem=b.WM_MEM_DEVICE)
                ms = float(ctx.last_stage_ms()[2]) / (P + new - 1)
                best = ms if best is None else min(best, ms)
            per_pos[label] = best
    finally:
        ctx.dev_free(d_mel)
    print(json.dumps(dict(model=name, recordings=N, audio_s=audio_s, conditioning=res, group_rows=N, group_P=P,
                          ragged_prompt_lengths=[len(p) for p in ragged], decode_ms_per_position=per_pos,
                          ragged_over_uniform=per_pos["ragged"] / per_pos["uniform"])))


def prompt_panel_probe():
    import ctypes
    SOT_PREV = 50361
    dbg = b.load_debug_library()
    ip = ctypes.POINTER(ctypes.c_int32)
    dbg.wmdbg_prompt_panel_plan.argtypes = [ctypes.c_int] * 5 + [ip]

    def plan(rows, P, sot):
        out = np.zeros(5, dtype=np.int32)
        assert dbg.wmdbg_prompt_panel_plan(rows, PPANEL, P, sot, -1, out.ctypes.data_as(ip)) == 0
        return [int(v) for v in out]   # P0, C, w', slices, panel steps per slice
    calls = []
    inner = ctx.transcribe_mel

    def counted(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k):
        t0 = time.perf_counter()
        r = inner(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k)
        calls.append(dict(rows=len(prompts), P=max(len(p) for p in prompts), wall=time.perf_counter() - t0,
                          decode_ms=float(ctx.last_stage_ms()[2]), gen=int(r.lens.max())))
        return r
    ctx.transcribe_mel = counted
    run = dict(condition_on_previous_text=True, sot_prev=SOT_PREV, logprob_threshold=None, compression_ratio_threshold=None,
               prompt_panel=PPANEL if PPANEL > 1 else None)
    ctx.transcribe_long(recs, **kw, **run)     # warm-up
    walls = []
    for _ in range(2):
        del calls[:]
        t0 = time.perf_counter()
        out = ctx.transcribe_long(recs, **kw, **run)
        walls.append(time.perf_counter() - t0)
    ctx.transcribe_mel = inner
    plans = [plan(c["rows"], c["P"], c["P"] - 3) for c in calls]   # (no_speech_prob is computed: P0 = <|startoftranscript|>)
    res = dict(model=name, recordings=N, audio_s=audio_s, prompt_panel=PPANEL, wall_s=walls, calls=len(calls),
               windows=sum(len(o["windows"]) for o in out), prompt_steps=sum(c["P"] for c in calls),
               generated_steps=sum(c["gen"] for c in calls), prompt_positions=sum(c["rows"] * c["P"] for c in calls),
               prefilled_positions=sum(c["rows"] * pl[0] for c, pl in zip(calls, plans) if pl[2]),
               panel_steps=sum(pl[3] * pl[4] for pl in plans),
               ordinary_prompt_steps=sum(c["P"] - (pl[0] if pl[2] else 0) for c, pl in zip(calls, plans)),
               decode_ms=sum(c["decode_ms"] for c in calls),
               tokens_digest=int(sum(int(t) * (i + 1) for o in out for s_ in o["segments"] for i, t in enumerate(s_["tokens"])) % 1000000007))
    # one uniform group: n_ctx / 2 + 3 prompt positions, one new token -- the decode stage is the prompt phase alone
    n_ctx = dims["n_text_ctx"]
    P = n_ctx // 2 + 3
    d_mel, offs, T = ctx.logmel_long(recs, n_mels=dims["n_mels"], device=True)
    rows = list(range(N))
    prng = np.random.default_rng(5)
    uniform = [[int(t) for t in prng.integers(0, 50000, size=P - 3)] + [SOT, 50259, TASK] for _ in rows]
    group = {}
    try:
        for width in sorted({1, PPANEL}):
            if PPANEL > 1:
                ctx.set_prompt_panel(width)
            best = None
            for _ in range(4):
                ctx.transcribe_mel(d_mel, offs[rows], T[rows], 0, [min(3000, int(t) - 3000) for t in T[rows]], uniform, 1,
                                   eot=-1, no_speech_token=NS, sot_tail=3, mem=b.WM_MEM_DEVICE)
                ms = float(ctx.last_stage_ms()[2])
                best = ms if best is None else min(best, ms)
            group[width] = best
    finally:
        ctx.dev_free(d_mel)
    pl = plan(N, P, P - 3)
    step_ms = group[1] / P
    res["group"] = dict(rows=N, P=P, decode_ms=group, ms_per_prompt_step=step_ms)
    if PPANEL > 1 and pl[2]:
        n_panel = pl[3] * pl[4]
        res["group"].update(P0=pl[0], slice_windows=pl[1], panel_width=pl[2], panel_steps=n_panel,
                            ms_per_panel_step=(group[PPANEL] - (P - pl[0]) * step_ms) / n_panel,
                            prompt_phase_speedup=group[1] / group[PPANEL])
    print(json.dumps(res))


def probe_vocab():
    import tempfile
    # GPT-2's byte alphabet: printable bytes stand for themselves, the others for U+0100 ...
    bs = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    b2u = {c: chr(c) for c in bs}
    b2u.update({c: chr(256 + i) for i, c in enumerate(c for c in range(256) if c not in bs)})
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vocab.json")
        with open(path, "w") as f:
            json.dump({"".join(b2u[c] for c in ((" w%d" % i) if i % 3 else ("x%d" % i)).encode()): i for i in range(EOT)}, f)
        return b.Vocab(path)


def words_probe():
    vocab = probe_vocab()
    calls = []
    inner = ctx.align_mel

    def counted(mel, mel_base, *a, **k):
        t0 = time.perf_counter()
        r = inner(mel, mel_base, *a, **k)
        calls.append(dict(rows=len(mel_base), wall=time.perf_counter() - t0, stage_ms=[float(v) for v in ctx.last_stage_ms()],
                          text_tokens=int((r[0] >= 0).sum()) - len(mel_base)))
        return r
    ctx.align_mel = counted
    keep = dict(logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, vocab=vocab)
    on = dict(keep, word_timestamps=True, no_timestamps=50363)
    ctx.transcribe_long(recs, **kw, **keep)
    ctx.transcribe_long(recs, **kw, **on)
    runs = [("off", keep, None), ("on", on, 1 if PANEL else None)] + ([("on_panel", on, PANEL)] if PANEL else [])
    if PANEL:
        ctx.set_teacher_panel(PANEL)
        ctx.transcribe_long(recs, **kw, **on)
    dec_ms = []   # wm_last_stage_ms[2] of the aligned decode calls of the run in progress
    if DECODE:
        dec = dict(keep, word_timestamps="decode")
        inner_dec = ctx.transcribe_mel_aligned

        def counted_dec(*a, **k):
            r = inner_dec(*a, **k)
            dec_ms.append(float(ctx.last_stage_ms()[2]))
            return r
        ctx.transcribe_mel_aligned = counted_dec
        ctx.transcribe_long(recs, **kw, **dec)
        runs.append(("decode", dec, None))
    walls = {label: [] for label, _, _ in runs}
    outs, stages = {}, {}
    for _ in range(3):
        for label, extra, width in runs:
            if width is not None:
                ctx.set_teacher_panel(width)
            del calls[:]
            del dec_ms[:]
            t0 = time.perf_counter()
            out = ctx.transcribe_long(recs, **kw, **extra)
            walls[label].append(time.perf_counter() - t0)
            outs[label] = out
            stages[label] = [sum(c["stage_ms"][i] for c in calls) for i in range(3)]
            if label == "off":
                windows_off = sum(len(o["windows"]) for o in out)
    ctx.align_mel = inner
    extra_out = {}
    if PANEL:
        ctx.set_teacher_panel(1)
        assert outs["on_panel"] == outs["on"], "the panel width changed the result"
        sp = stages["on_panel"]
        extra_out = dict(teacher_panel=PANEL, on_panel_over_off=float(np.median(walls["on_panel"]) / np.median(walls["off"])),
                         on_panel_over_on=float(np.median(walls["on_panel"]) / np.median(walls["on"])),
                         align_stage_ms_panel=dict(encoder_cross_kv=sp[0], teacher_forced=sp[1], alignment_dtw=sp[2]))
    if DECODE:
        ctx.transcribe_mel_aligned = inner_dec
        tok = lambda o: [[w["tokens"] for w in r["windows"]] for r in o]   # noqa: E731
        same_windows = tok(outs["decode"]) == tok(outs["off"])   # (the word-driven seek may cut other windows than `off`)
        med = {k: float(np.median(v)) for k, v in walls.items()}
        extra_out.update(decode_over_off=med["decode"] / med["off"], decode_over_on=med["decode"] / med["on"],
                         decode_windows=sum(len(o["windows"]) for o in outs["decode"]),
                         decode_words=sum(len(s["words"]) for o in outs["decode"] for s in o["segments"]),
                         decode_same_windows_as_off=same_windows, decode_loop_ms=sum(dec_ms), decode_calls=len(dec_ms))
        if PANEL:
            extra_out["decode_over_on_panel"] = med["decode"] / med["on_panel"]
    out = outs["on"]
    stage = stages["on"]
    print(json.dumps(dict(model=name, recordings=N, audio_s=audio_s, wall_s=walls,
                          median_wall_s={k: float(np.median(v)) for k, v in walls.items()},
                          on_over_off=float(np.median(walls["on"]) / np.median(walls["off"])),
                          windows_off=windows_off, windows_on=sum(len(o["windows"]) for o in out),
                          words=sum(len(s["words"]) for o in out for s in o["segments"]),
                          align_calls=len(calls), align_rows=sum(c["rows"] for c in calls),
                          align_text_tokens=sum(c["text_tokens"] for c in calls),
                          align_wall_s=sum(c["wall"] for c in calls),
                          align_stage_ms=dict(encoder_cross_kv=stage[0], teacher_forced=stage[1], alignment_dtw=stage[2]),
                          **extra_out)))


def reuse_probe():
    vocab = probe_vocab()
    log = []   # (call, rows, wm_last_stage_ms) of every model call of the run in progress

    def counted(fn_name, rows_of):
        inner = getattr(ctx, fn_name)

        def f(*a, **k):
            r = inner(*a, **k)
            log.append((fn_name, rows_of(a), [float(v) for v in ctx.last_stage_ms()]))
            return r
        setattr(ctx, fn_name, f)
    counted("transcribe_mel", lambda a: len(a[1]))
    counted("align_mel", lambda a: len(a[1]))
    counted("encode_windows", lambda a: len(a[1]))
    counted("transcribe_windows", lambda a: len(a[1]))
    counted("align_windows", lambda a: len(a[1]))
    window_bytes = dims["n_text_layer"] * 2 * 1500 * dims["n_text_state"] * 2
    keep = dict(logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
    configs = (("fallback", dict(vocab=vocab)),
               ("words_no_fallback", dict(keep, vocab=vocab, word_timestamps=True, no_timestamps=50363)))
    for label, extra in configs:
        outs = {}
        for reuse in (False, True):
            outs[reuse] = ctx.transcribe_long(recs, **kw, **extra, reuse_encoder=reuse)     # warm-up of each
        assert outs[True] == outs[False], "reuse_encoder changed the result"
        walls, logs = {False: [], True: []}, {}
        for _ in range(3):
            for reuse in (False, True):
                del log[:]
                t0 = time.perf_counter()
                ctx.transcribe_long(recs, **kw, **extra, reuse_encoder=reuse)
                walls[reuse].append(time.perf_counter() - t0)
                logs[reuse] = list(log)

        def total(reuse, call, i):
            return sum(c[2][i] for c in logs[reuse] if c[0] == call)

        def rows(reuse, call):
            return sum(c[1] for c in logs[reuse] if c[0] == call)
        off_rows = rows(False, "transcribe_mel") + rows(False, "align_mel")
        off_enc_ms = total(False, "transcribe_mel", 1) + total(False, "align_mel", 0)   # (align: [0] = staging + encoder + K/V)
        on_rows = rows(True, "transcribe_windows") + rows(True, "align_windows")
        gather_ms = total(True, "transcribe_windows", 0) + total(True, "align_windows", 0)
        enc_rows = rows(True, "encode_windows")
        res = dict(config=label, model=name, recordings=N, audio_s=audio_s,
                   wall_s=dict(off=walls[False], on=walls[True]),
                   median_wall_s=dict(off=float(np.median(walls[False])), on=float(np.median(walls[True]))),
                   on_over_off=float(np.median(walls[True]) / np.median(walls[False])),
                   windows=sum(len(o["windows"]) for o in outs[False]),
                   off=dict(decode_calls=sum(c[0] == "transcribe_mel" for c in logs[False]), decode_rows=rows(False, "transcribe_mel"),
                            align_calls=sum(c[0] == "align_mel" for c in logs[False]), align_rows=rows(False, "align_mel"),
                            decode_stage_ms=[total(False, "transcribe_mel", i) for i in range(3)],
                            align_stage_ms=[total(False, "align_mel", i) for i in range(3)],
                            encoder_cross_kv_ms_per_window=off_enc_ms / max(off_rows, 1)),
                   on=dict(encode_calls=sum(c[0] == "encode_windows" for c in logs[True]), encode_rows=enc_rows,
                           encode_stage_ms=[total(True, "encode_windows", i) for i in range(3)],
                           encode_ms_per_window=total(True, "encode_windows", 1) / max(enc_rows, 1),
                           decode_rows=rows(True, "transcribe_windows"), align_rows=rows(True, "align_windows"),
                           decode_stage_ms=[total(True, "transcribe_windows", i) for i in range(3)],
                           align_stage_ms=[total(True, "align_windows", i) for i in range(3)],
                           gather_ms=gather_ms, gather_rows=on_rows, gather_ms_per_window=gather_ms / max(on_rows, 1),
                           gather_gb_per_s=2 * window_bytes * on_rows / max(gather_ms, 1e-9) / 1e6,
                           set_bytes_per_window=window_bytes))
        print(json.dumps(res), flush=True)


def fallback_probe():
    calls = []
    inner = ctx.transcribe_mel

    def counted(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k):
        r = inner(mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **k)
        calls.append((len(prompts), max(len(p) for p in prompts) + int(r.lens.max())))
        return r
    ctx.transcribe_mel = counted
    rounds = []
    round_rows = b._RoundRows

    class CountedRound(round_rows):   # one row source per round: the loop's own count, whatever parallel_clips bounds
        def __init__(self, *a, **k):
            rounds.append(1)
            round_rows.__init__(self, *a, **k)
    b._RoundRows = CountedRound
    extra = {}
    if SHARE < 1.0:   # a calibration run: the S-quantile of the temperature-0 avg_logprob of every window
        cal = ctx.transcribe_long(recs, temperatures=(0.0,), logprob_threshold=None, compression_ratio_threshold=None,
                                  no_speech_threshold=None, **kw)
        lps = [sg["avg_logprob"] for o in cal for sg in {g["seek"]: g for g in o["segments"]}.values()]
        extra = dict(logprob_threshold=float(np.quantile(lps, SHARE)), compression_ratio_threshold=None, no_speech_threshold=None)
    modes = ["lockstep"] if FALLBACK == "lockstep" else ["lockstep", "deferred"]
    res = {m: dict(wall_s=[]) for m in modes}
    outs = {}
    for m in modes:
        ctx.transcribe_long(recs, fallback=m, **kw, **extra)     # warm-up of each
    for _ in range(3):
        for m in modes:
            del calls[:]
            del rounds[:]
            t0 = time.perf_counter()
            outs[m] = ctx.transcribe_long(recs, fallback=m, **kw, **extra)
            res[m]["wall_s"].append(time.perf_counter() - t0)
            res[m].update(rounds=len(rounds), decode_calls=len(calls), positions_stepped=sum(c[1] for c in calls),
                          row_positions=sum(c[0] * c[1] for c in calls))
    for m in modes:
        res[m]["median_wall_s"] = float(np.median(res[m]["wall_s"]))
        res[m]["audio_s_per_s"] = audio_s / res[m]["median_wall_s"]
    ctx.transcribe_mel = inner
    b._RoundRows = round_rows
    strip = lambda out: [dict(o, windows=[{k: v for k, v in w.items() if k != "round"} for w in o["windows"]]) for o in out]  # noqa: E731
    if len(modes) == 2:
        assert strip(outs["lockstep"]) == strip(outs["deferred"])
        res["deferred_over_lockstep"] = res["deferred"]["median_wall_s"] / res["lockstep"]["median_wall_s"]
    temps = [w["temperatures"] for o in outs["lockstep"] for w in o["windows"]]
    print(json.dumps(dict(model=name, recordings=N, audio_s=audio_s, share_asked=SHARE, thresholds=extra, windows=len(temps),
                          windows_fell_back=sum(len(t) > 1 for t in temps), attempts=sum(len(t) for t in temps), **res)))


def rows_position_probe():
    P, new = 3, 64
    d_mel, offs, T = ctx.logmel_long(recs, n_mels=dims["n_mels"], device=True)
    rows = list(range(N))
    mixed = [(0.0, 0.8, 0.0, 1.0)[i % 4] for i in rows]
    variants = (("scalar", {}), ("map_one_pair", dict(row_temperatures=[0.8] * N, row_seeds=[5] * N)),
                ("map_mixed", dict(row_temperatures=mixed, row_seeds=[5 + i for i in rows])))
    out, profile = {}, {}
    try:
        for rules in (False, True):
            if rules:
                ctx.set_sampling_rules(50, 0.9, 0.0)
            best = {}
            for _ in range(4):
                for label, k in variants:
                    ctx.transcribe_mel(d_mel, offs[rows], T[rows], 0, [min(3000, int(t) - 3000) for t in T[rows]],
                                       [SOT, 50259, TASK], new, eot=-1, no_speech_token=NS, temperature=0.8, seed=5,
                                       mem=b.WM_MEM_DEVICE, **k)
                    ms = float(ctx.last_stage_ms()[2]) / (P + new - 1)
                    best[label] = ms if label not in best else min(best[label], ms)
            out["rules_on" if rules else "rules_off"] = best
            # per-launch HIP-event times of the two launches that read the table (eager launches: every launch bracketed by events)
            ctx.profile_enable(True)
            fam = {}
            for label, k in variants:
                for _ in range(2):
                    ctx.profile_reset()
                    ctx.transcribe_mel(d_mel, offs[rows], T[rows], 0, [min(3000, int(t) - 3000) for t in T[rows]],
                                       [SOT, 50259, TASK], new, eot=-1, no_speech_token=NS, temperature=0.8, seed=5,
                                       mem=b.WM_MEM_DEVICE, **k)
                fam[label] = {q: round(v["ms"] / v["n"] * 1e3, 2) for q, v in ctx.profile().items()
                              if isinstance(v, dict) and v.get("n") and ("logits" in q or "sample_trunc" in q)}
            ctx.profile_enable(False)
            profile["rules_on" if rules else "rules_off"] = fam
    finally:
        ctx.set_sampling_rules()
        ctx.dev_free(d_mel)
    print(json.dumps(dict(model=name, rows=N, positions=P + new - 1, decode_ms_per_position=out, profile_us_per_launch=profile)))


if FALLBACK is not None:
    fallback_probe()
    sys.exit(0)
if ROWS_POSITION:
    rows_position_probe()
    sys.exit(0)
if CONDITION:
    condition_probe()
    sys.exit(0)
if PPANEL is not None:
    prompt_panel_probe()
    sys.exit(0)
if REUSE:
    reuse_probe()
    sys.exit(0)
if WORDS:
    words_probe()
    sys.exit(0)
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
