"""CPU tests of prompt conditioning and ragged prompts (binding.conditioned_prompt / conditioned_history, the
condition_on_previous_text loop of binding.transcribe_long, and the host-side right-alignment of wm_transcribe_mel_ragged).
openai-whisper's rule restated, from whisper/transcribe.py and whisper/decoding.py (DecodingTask._get_initial_tokens):

    all_tokens = []; prompt_reset_since = 0
    if initial_prompt is not None:
        all_tokens.extend(initial_prompt_tokens)
    while seek < content_frames:
        decode_options["prompt"] = all_tokens[prompt_reset_since:]
        result = decode_with_fallback(mel_segment)
        if should_skip:
            seek += segment_size
            continue
        ... current_segments ...
        all_tokens.extend([token for segment in current_segments for token in segment["tokens"]])
        if not condition_on_previous_text or result.temperature > 0.5:
            prompt_reset_since = len(all_tokens)

    tokens = list(sot_sequence)
    if prompt:
        prompt_tokens = prompt
        tokens = [tokenizer.sot_prev] + prompt_tokens[-(n_ctx // 2 - 1):] + tokens
"""
import ctypes
import importlib

import numpy as np
import pytest

B = importlib.import_module("openai_whisper_coreml_amd.binding")

SOT, LANG, TASK, SOT_PREV, NS, TSB, EOT = 50258, 50259, 50359, 50361, 50362, 50364, 50257


def expected_prompts(windows, segments, initial, sot_sequence, sot_prev, n_ctx, reset_above=0.5):
    """The literal rule above, replayed over the `windows` and `segments` records of one recording of a transcribe_long
    result: the prompt every window must have had, in order."""
    all_tokens = [int(t) for t in initial]
    prompt_reset_since = 0
    out = []
    for w in windows:
        prompt = all_tokens[prompt_reset_since:]
        tokens = list(sot_sequence)
        if prompt:
            tokens = [sot_prev] + prompt[-(n_ctx // 2 - 1):] + tokens
        out.append(tokens)
        if w["skipped"]:
            continue
        current = [s for s in segments if s["seek"] == w["seek"]]
        all_tokens.extend([t for s in current for t in s["tokens"]])
        if w["temperatures"][-1] > reset_above:
            prompt_reset_since = len(all_tokens)
    return out


def _replay(initial, steps, n_ctx, reset_above=0.5):
    """Drive the two helpers over `steps` = [(segment token lists, temperature, skipped)]: the prompts they give."""
    all_tokens, since = list(initial), 0
    got = []
    for seg_tokens, temp, skipped in steps:
        got.append(B.conditioned_prompt(all_tokens, since, [SOT, LANG, TASK], SOT_PREV, n_ctx))
        before = list(all_tokens)
        all_tokens, since = B.conditioned_history(all_tokens, since, [dict(tokens=t) for t in seg_tokens], temp, skipped,
                                                  reset_above)
        if skipped:
            assert all_tokens == before
    return got


def _records(steps):
    windows, segments = [], []
    for i, (seg_tokens, temp, skipped) in enumerate(steps):
        windows.append(dict(seek=100 * i, temperatures=[0.0, temp] if temp > 0 else [0.0], skipped=skipped))
        if not skipped:
            segments += [dict(seek=100 * i, tokens=list(t)) for t in seg_tokens]
    return windows, segments


@pytest.mark.parametrize("n_ctx", [448, 64])
def test_prompt_helpers_follow_the_literal_rule(n_ctx):
    rng = np.random.default_rng(n_ctx)
    toks = lambda n: [int(t) for t in rng.integers(0, 50000, size=n)]
    half = n_ctx // 2 - 1
    cases = {
        "empty history": ([], [([toks(5)], 0.0, False)]),
        "truncation": ([], [([toks(half), toks(9)], 0.0, False), ([toks(3)], 0.0, False), ([toks(2)], 0.0, False)]),
        "initial prompt until the first reset": (toks(6), [([toks(4)], 0.0, False), ([toks(4)], 0.8, False),
                                                           ([toks(4)], 0.0, False), ([toks(2)], 0.0, False)]),
        "reset above the threshold only": ([], [([toks(4)], 0.5, False), ([toks(4)], 0.6, False), ([toks(4)], 0.0, False)]),
        "skipped window": (toks(3), [([toks(4)], 0.0, False), ([toks(7)], 1.0, True), ([toks(4)], 0.0, False)]),
        "cleared segments": ([], [([toks(4), [], toks(2)], 0.0, False), ([[]], 0.0, False), ([toks(1)], 0.0, False)]),
        "long initial prompt": (toks(n_ctx), [([toks(4)], 0.0, False), ([toks(4)], 0.0, False)]),
    }
    for name, (initial, steps) in cases.items():
        got = _replay(initial, steps, n_ctx)
        want = expected_prompts(*_records(steps), initial, [SOT, LANG, TASK], SOT_PREV, n_ctx)
        assert got == want, name
        assert all(len(p) <= n_ctx // 2 + 3 for p in got), name
    # the cases show what they are named for
    got = _replay([], cases["empty history"][1], n_ctx)
    assert got[0] == [SOT, LANG, TASK]
    got = _replay(*cases["truncation"], n_ctx)
    assert len(got[1]) == n_ctx // 2 + 3 and got[1][0] == SOT_PREV and got[1][1:-3] == (
        cases["truncation"][1][0][0][0] + cases["truncation"][1][0][0][1])[-half:]
    init, steps = cases["initial prompt until the first reset"]
    got = _replay(init, steps, n_ctx)
    assert got[0][1:1 + len(init)] == init and got[1][1:1 + len(init)] == init
    assert got[2] == [SOT, LANG, TASK] and got[3] == [SOT_PREV] + steps[2][0][0] + [SOT, LANG, TASK]
    got = _replay(*cases["reset above the threshold only"], n_ctx)
    assert len(got[1]) == 1 + 4 + 3 and got[2] == [SOT, LANG, TASK]     # 0.5 is not above 0.5; 0.6 is
    init, steps = cases["skipped window"]
    got = _replay(init, steps, n_ctx)
    assert got[2] == got[1]     # neither the tokens nor the temperature of a skipped window count
    # a threshold of its own
    assert _replay([], [([toks(2)], 0.9, False), ([toks(2)], 0.0, False)], n_ctx, reset_above=2.0)[1][0] == SOT_PREV


# ---------------------------------------------------------------- transcribe_long on a fake context
class FakeCtx:
    """Canned logmel_long and transcribe_mel (the language is given, so nothing is detected): every window decodes to
    [<|0.00|>, two text tokens derived from (recording id, window ordinal), <|10.00|>, <|10.00|>, eot]: one segment of four
    tokens, and the seek advances by 10 s."""

    def __init__(self, n_ctx=64, fall_back=()):
        self.dims = dict(n_text_ctx=n_ctx, n_mels=80, n_vocab=51865)
        self.calls = []
        self.fall_back = set(fall_back)   # (recording id, window ordinal) whose decodes below temperature 0.6 are rejected

    def set_timestamp_rules(self, *a):
        pass

    def logmel_long(self, recordings, n_mels=80, device=False):
        T = np.array([(len(r) + 480000) // 160 for r in recordings], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(T.astype(np.int64) * n_mels)])
        return ctypes.c_void_p(4096), offs, T

    def dev_free(self, p):
        pass

    def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, eot=-1, temperature=0.0, seed=0,
                       no_speech_token=-1, sot_index=0, sample_ids=None, mem=0, budgets=None, prompt_len=None,
                       sot_tail=None):
        self.calls.append(dict(prompts=[list(map(int, p)) for p in prompts], max_new=max_new, temperature=temperature,
                               sot_tail=sot_tail, sot_index=sot_index, sample_ids=list(sample_ids)))
        n = len(sample_ids)
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        for i, sid in enumerate(sample_ids):
            rec, ordinal = int(sid) & 0xFFFF, int(sid) >> 16
            body = [TSB, 1000 + 10 * rec + ordinal, 2000 + ordinal, TSB + 500, TSB + 500, eot]
            toks[i, :len(body)] = body
            lens[i] = len(body)
            bad = temperature < 0.55 and (rec, ordinal) in self.fall_back
            lp[i, :len(body)] = -5.0 if bad else -0.1
        return B.TranscribeResult(toks, lens, lp, np.full(n, 0.01, dtype=np.float32), eot)


def _fake_kw(**extra):
    kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TSB, no_speech_token=NS, language=LANG, sot_prev=SOT_PREV,
              compression_ratio_threshold=None)
    kw.update(extra)
    return kw


def test_transcribe_long_passes_the_helpers_prompts_in_one_ragged_call_per_round():
    n_ctx = 64
    recs = [np.zeros(16000 * s, np.float32) for s in (25, 12, 38)]
    seeds = [[], [7, 8], list(range(100, 100 + n_ctx))]
    ctx = FakeCtx(n_ctx, fall_back={(0, 1)})
    out = B.transcribe_long(ctx, recs, condition_on_previous_text=True, initial_prompt_tokens=seeds, **_fake_kw())
    want_new = min(n_ctx // 2, n_ctx - (n_ctx // 2 + 3))
    assert want_new == 29 and min(448 // 2, 448 - (448 // 2 + 3)) == 221
    assert all(c["max_new"] == want_new and c["sot_tail"] == 3 for c in ctx.calls)
    # every window's prompt is the literal rule's, from the records alone
    for r, o in enumerate(out):
        want = expected_prompts(o["windows"], o["segments"], seeds[r], [SOT, LANG, TASK], SOT_PREV, n_ctx)
        assert [w["prompt"] for w in o["windows"]] == want, r
        assert [w["prompt_len"] for w in o["windows"]] == [len(p) for p in want]
    assert [len(o["windows"]) for o in out] == [3, 2, 4]
    # round 1: the three recordings in ONE call, prompts of 3, 6 and n_ctx // 2 + 3 tokens
    first = ctx.calls[0]
    assert [len(p) for p in first["prompts"]] == [3, 6, n_ctx // 2 + 3] and first["temperature"] == 0.0
    assert first["prompts"] == [o["windows"][0]["prompt"] for o in out]
    # the rejected window was decoded again at 0.2, 0.4 and 0.6 (alone), fed its prompt every time, and -- its final
    # temperature being above 0.5 -- reset the recording's history
    again = [c for c in ctx.calls if c["temperature"] > 0]
    assert [c["temperature"] for c in again] == [0.2, 0.4, 0.6]
    assert all(c["prompts"] == [out[0]["windows"][1]["prompt"]] for c in again)
    assert out[0]["windows"][1]["temperatures"] == [0.0, 0.2, 0.4, 0.6] and out[0]["windows"][2]["prompt"] == [SOT, LANG, TASK]
    assert out[0]["windows"][1]["prompt"][0] == SOT_PREV and out[0]["windows"][1]["prompt"][1:-3] == out[0]["segments"][0]["tokens"]
    # a threshold above every temperature: the sampled window's tokens feed the next prompt
    ctx2 = FakeCtx(n_ctx, fall_back={(0, 1)})
    out2 = B.transcribe_long(ctx2, recs, condition_on_previous_text=True, initial_prompt_tokens=seeds,
                             prompt_reset_on_temperature=2.0, **_fake_kw())
    assert out2[0]["windows"][2]["prompt"][0] == SOT_PREV and len(out2[0]["windows"][2]["prompt"]) > 3


def test_transcribe_long_without_conditioning_keeps_its_prompts():
    recs = [np.zeros(16000 * s, np.float32) for s in (25, 12)]
    ctx = FakeCtx(64)
    out = B.transcribe_long(ctx, recs, initial_prompt_tokens=[5, 6], **_fake_kw())
    head = [SOT_PREV, 5, 6, SOT, LANG, TASK]
    assert all(c["max_new"] == 32 and c["sot_index"] == 3 and c["sot_tail"] is None for c in ctx.calls)
    assert all(p == head for c in ctx.calls for p in c["prompts"])
    assert all(w["prompt"] == head and w["prompt_len"] == 6 for o in out for w in o["windows"])
    # one list per recording: each heads every window of its own recording
    ctx = FakeCtx(64)
    out = B.transcribe_long(ctx, recs, initial_prompt_tokens=[[], [9]], **_fake_kw())
    assert all(w["prompt"] == [SOT, LANG, TASK] for w in out[0]["windows"])
    assert all(w["prompt"] == [SOT_PREV, 9, SOT, LANG, TASK] for w in out[1]["windows"])
    assert all(c["max_new"] == 32 and c["sot_tail"] == 3 for c in ctx.calls)
    with pytest.raises(ValueError):
        B.transcribe_long(FakeCtx(64), recs, condition_on_previous_text=True, **_fake_kw(sot_prev=None))
    with pytest.raises(ValueError):
        B.transcribe_long(FakeCtx(64), recs, initial_prompt_tokens=[[1], [2], [3]], **_fake_kw())


# ---------------------------------------------------------------- the right-aligned prompt table
def right_align_np(prompts, prompt_len, b0, Bg):
    """Rows [b0, b0 + Bg) right-aligned to the group's own longest prompt: table [P][Bg], offsets [Bg].  The positions in
    front of a prompt repeat its first token."""
    lens = [int(n) for n in prompt_len[b0:b0 + Bg]]
    P = max(lens)
    table = np.zeros((P, Bg), dtype=np.int32)
    off = np.array([P - n for n in lens], dtype=np.int32)
    for b in range(Bg):
        row = prompts[b0 + b]
        table[:off[b], b] = row[0]
        table[off[b]:, b] = row[:lens[b]]
    return P, table, off


def _right_align(lib, prompts, prompt_len, b0, Bg):
    stride = prompts.shape[1]
    table = np.full(stride * Bg, -7, dtype=np.int32)
    off = np.full(Bg, -7, dtype=np.int32)
    vp = ctypes.c_void_p
    lib.wmdbg_right_align.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    P = lib.wmdbg_right_align(prompts.ctypes.data_as(vp), stride, prompt_len.ctypes.data_as(vp), b0, Bg,
                              table.ctypes.data_as(vp), off.ctypes.data_as(vp))
    assert np.all(table[P * Bg:] == -7)
    return P, table[:P * Bg].reshape(P, Bg), off


def test_right_alignment_of_a_decode_group(pkg):
    lib = pkg.binding.load_debug_library()
    rng = np.random.default_rng(12)
    n_rows, stride = 300, 40
    prompts = rng.integers(0, 51865, size=(n_rows, stride)).astype(np.int32)
    plen = rng.integers(1, stride + 1, size=n_rows).astype(np.int32)
    for Bg in (1, 16, 17, 128):
        for b0 in (0, 5, n_rows - Bg):
            P, table, off = _right_align(lib, prompts, plen, b0, Bg)
            wP, wtable, woff = right_align_np(prompts, plen, b0, Bg)
            assert P == wP == plen[b0:b0 + Bg].max() and np.array_equal(off, woff) and np.array_equal(table, wtable)
            assert off.min() == 0 and np.all(table[-1] == prompts[np.arange(b0, b0 + Bg), plen[b0:b0 + Bg] - 1])
    # lengths that differ only in rows of ANOTHER group do not change a group's P or table
    plen2 = plen.copy()
    plen2[:100] = 3
    plen2[100 + 17:] = stride
    plen3 = plen2.copy()
    plen3[:100] = stride
    plen3[100 + 17:] = 1
    a = _right_align(lib, prompts, plen2, 100, 17)
    c = _right_align(lib, prompts, plen3, 100, 17)
    assert a[0] == c[0] == plen[100:117].max() and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
