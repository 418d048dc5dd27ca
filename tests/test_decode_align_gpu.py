"""GPU tests of word timestamps from the decode's own pass: wm_transcribe_mel_aligned / wm_transcribe_windows_aligned (the
decode keeps the alignment heads' cross-attention queries; each group ends with the alignment kernels and the DTW) and
transcribe_long(word_timestamps="decode") on top.  Yardsticks: the EXISTING wm_transcribe_mel / wm_transcribe_mel_ragged for
the tokens (bit for bit), tests/test_align_gpu.py's fp32 oracle forward with the numpy restatement of find_alignment's
post-processing (tests/test_align_cpu.py) for the cost matrix, numpy's DTW on the GPU's own matrix for the start frames."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from test_align_cpu import median_filter, start_frames, zscore
from test_align_gpu import GATE_TINY, dbg, default_heads, oracle_forward  # noqa: F401  (dbg: module fixture)
from test_longform_gpu import EOT2, NS, SOT, TSB, _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import prod_vocab  # noqa: F401  (fixture)
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_transcribe_options_gpu import EOT, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
NO_TS, NS_TOK = 889, 899
SOT_SEQ = [10, 21, 5]
NEW = 24
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    out = os.environ.get("WM_MEASURED_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_align_measured.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def mel3(dbg):
    _, _, ctx = dbg
    return ctx.logmel(tones(3), out_dtype=np.float32)


def _base(n):
    return (np.arange(n, dtype=np.int64) % 3) * 240000


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint32)


def _same_decode(r, plain, what):
    """an AlignedResult against transcribe_mel_raw's (tokens, lens, logprobs, no_speech): the raw bits"""
    for name, x, y in zip(("tokens", "lens", "logprobs", "no_speech"), (r.tokens, r.lens, r.logprobs, r.no_speech_prob), plain):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert np.array_equal(_bits(x), _bits(y)), (what, name)


def _plain(ctx, b, mel, base, prompts, n_frames=3000, T=0.0, seed=77, sot_index=0, sot_tail=None, ids=None, budgets=None, eot=EOT,
           new=NEW):
    opts = b.wm_decode_opts(T, seed, NS_TOK, sot_index)
    return ctx.transcribe_mel_raw(mel, base, 3000, 0, n_frames, prompts, new, eot, opts, sample_ids=ids, logprobs=True,
                                  no_speech=True, budgets=budgets, sot_tail=sot_tail)


def _aligned(ctx, mel, base, prompts, n_frames=3000, T=0.0, seed=77, sot_index=0, sot_tail=None, ids=None, budgets=None, eot=EOT,
             new=NEW, **kw):
    return ctx.transcribe_mel_aligned(mel, base, 3000, 0, n_frames, prompts, new, eot=eot, temperature=T, seed=seed,
                                      no_speech_token=NS_TOK, sot_index=sot_index, sample_ids=ids, budgets=budgets,
                                      sot_tail=sot_tail, **kw)


def _ragged_prompts(lens=(3, 5, 9), seed=4):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, EOT, size=n - 3)] + SOT_SEQ for n in lens]


# ---------------------------------------------------------------- 1. the tokens are untouched
CASES_1 = {
    "uniform": dict(),
    "ragged-budgets": dict(ragged=True, budgets=[1, 7, 24]),
    "sampled": dict(T=0.7, ids=np.array([(3 << 16) | 17, 5, 70000], dtype=np.uint32)),
    "rules": dict(rules=True),
}


@pytest.mark.parametrize("case", sorted(CASES_1))
def test_tokens_logprobs_and_no_speech_are_the_plain_call_s_bits(dbg, pkg, mel3, case):
    _, _, ctx = dbg
    c = dict(CASES_1[case])
    ragged, rules = c.pop("ragged", False), c.pop("rules", False)
    prompts = _ragged_prompts() if ragged else np.array([SOT_SEQ] * 3, dtype=np.int32)
    if ragged:
        c["sot_tail"] = 3
    if rules:   # timestamp rules + suppress lists + no_repeat_ngram_size 3 + one banned sequence
        _rules(ctx)
        ctx.set_repetition_rules(1.0, 3, EOT)
        first = _plain(ctx, pkg.binding, mel3, _base(3), prompts)
        t0 = [int(t) for t in first[0][0, :first[1][0]]]
        i = next(k for k in range(1, len(t0)) if t0[k] < EOT)
        ban = (t0[i - 1], t0[i])   # what row 0 would generate: the ban changes the stream
        ctx.set_sequence_bias({ban: float("-inf")}, eot=EOT)
    try:
        want = _plain(ctx, pkg.binding, mel3, _base(3), prompts, **c)
        got = _aligned(ctx, mel3, _base(3), prompts, **c)
        _same_decode(got, want, case)
        if rules:
            assert not np.array_equal(first[0], want[0]) and (want[0] >= 900).any()   # the ban bit, timestamps occur
        if ragged:
            assert int(got.lens[0]) == 1 and 1 <= int(got.lens[1]) <= 7 and 1 <= int(got.lens[2]) <= 24
        for b in range(3):   # the start frames of every row are a monotone path that ends at M
            n = int(got.lens[b])
            sf = got.start_frames[b]
            assert sf[n] == 1500 and np.all(sf[n + 1:] == -1) and np.all(np.diff(sf[:n + 1]) >= 0) and sf[0] >= 0, (case, b, sf)
    finally:
        if rules:
            ctx.set_sequence_bias(None)
            ctx.set_repetition_rules(1.0, 0, EOT)
            _rules(ctx, False)


# ---------------------------------------------------------------- 2. + 3. the cost matrix against the fp32 oracle, the DTW exactly
def decode_matrix(qk, n_frames, width, qk_scale, n_rows):
    """Steps 2 - 5 over ALL rows of qk [J][R][>= M] (= q.k / 8), f32 throughout; the last n_rows rows, negated"""
    w = torch.as_tensor(np.asarray(qk, dtype=np.float32))[:, :, : n_frames // 2]
    w = (w * qk_scale).softmax(dim=-1).numpy()
    w = median_filter(zscore(w), width)
    return -np.asarray(w).mean(axis=0)[-n_rows:]


def _window_xa(ctx, mel_row, n_frames):
    win = np.zeros((1, 80, 3000), dtype=np.float32)
    win[0, :, :n_frames] = mel_row[:, :n_frames]
    return ctx.encode_mel(win)[0]


def _check_matrix(ctx, sd, dims, mel, r, prompts, sot_at, n_frames, width, key, qk_scale=1.0):
    """Every row of the call: rel-L2 of the captured matrix against the oracle (gate GATE_TINY), its extent, and the DTW"""
    heads = default_heads(dims)
    for b in range(len(prompts)):
        n, nf = int(r.lens[b]), int(n_frames[b])
        M = nf // 2
        sf, mat = r.start_frames[b], r.matrix[b]
        assert n >= 1, (key, b)
        prompt = [int(t) for t in prompts[b]]
        seq = prompt + [int(t) for t in r.tokens[b, :n - 1]]     # the decoder's inputs: the last generated token is never fed
        _, qk = oracle_forward(sd, dims, seq, _window_xa(ctx, mel[b], nf))
        want = decode_matrix(np.stack([qk[l, h, sot_at[b]:] for l, h in heads]), nf, width, qk_scale, n)
        assert want.shape == (n, M)
        got = mat[:n, :M]
        assert np.all(mat[n:] == 0) and np.all(mat[:, M:] == 0), (key, b)
        e = R.rel_l2(got, want)
        _note(key, e)
        print("decode alignment %s row %d (len %d, M %d, width %d): rel-L2 %.5f (gate %.3f)" % (key, b, n, M, width, e, GATE_TINY))
        assert e <= GATE_TINY, (key, b, e)
        assert sf[:n].tolist() == start_frames(got).tolist(), (key, b)     # exact, on the GPU's own matrix
        assert sf[n] == M and np.all(sf[n + 1:] == -1), (key, b)
        d = np.abs(start_frames(want) - sf[:n])
        _note(key + "_frame_median", np.median(d))


def test_cost_matrix_no_timestamps_prompt_against_the_oracle(dbg, mel3):
    """Measured on an MI355X: see DESIGN.md section 16 (rel-L2 per case, gate 0.06)."""
    dims, sd, ctx = dbg
    prompts = np.array([SOT_SEQ + [NO_TS]] * 3, dtype=np.int32)
    r = _aligned(ctx, mel3, _base(3), prompts, capture_matrix=True)
    _check_matrix(ctx, sd, dims, mel3, r, prompts, [0] * 3, [3000] * 3, 7, "a_no_timestamps")


def test_cost_matrix_with_timestamp_tokens_against_the_oracle(dbg, mel3):
    dims, sd, ctx = dbg
    _rules(ctx)
    try:
        prompts = _ragged_prompts()
        r = _aligned(ctx, mel3, _base(3), prompts, sot_tail=3, capture_matrix=True)
        assert any((r.tokens[b, :r.lens[b]] >= 900).any() for b in range(3))     # timestamp ids among g
        _check_matrix(ctx, sd, dims, mel3, r, prompts, [len(p) - 3 for p in prompts], [3000] * 3, 7, "b_timestamp_rules")
    finally:
        _rules(ctx, False)


@pytest.mark.parametrize("width", [1, 7])
def test_cost_matrix_short_windows_against_the_oracle(dbg, mel3, width):
    """n_frames 1234, and a window of 4 frames: M = 2 is narrower than the filter (no filtering, as openai-whisper)"""
    dims, sd, ctx = dbg
    prompts = np.array([SOT_SEQ] * 3, dtype=np.int32)
    nf = [1234, 1234, 4]
    r = _aligned(ctx, mel3, _base(3), prompts, n_frames=nf, medfilt_width=width, capture_matrix=True)
    _check_matrix(ctx, sd, dims, mel3, r, prompts, [0] * 3, nf, width, "c_short_windows_w%d" % width)


# ---------------------------------------------------------------- 4. a row depends on the row alone
def test_rows_alone_together_and_across_groups_give_the_same_bits(dbg, pkg, mel3):
    _, _, ctx = dbg
    prompts = _ragged_prompts()
    nf = [3000, 1234, 601]
    together = _aligned(ctx, mel3, _base(3), prompts, n_frames=nf, sot_tail=3)
    for b in range(3):
        alone = _aligned(ctx, mel3, _base(3)[b:b + 1], prompts[b:b + 1], n_frames=nf[b:b + 1], sot_tail=3)
        assert np.array_equal(alone.start_frames[0], together.start_frames[b]), b
        # ... and the same row in a UNIFORM call: its own prompt, <|startoftranscript|> counted from the front
        uni = _aligned(ctx, mel3, _base(3)[b:b + 1], np.array([prompts[b]], dtype=np.int32), n_frames=nf[b:b + 1],
                       sot_index=len(prompts[b]) - 3)
        assert np.array_equal(uni.start_frames[0], together.start_frames[b]), b
        _same_decode(uni, [x[b:b + 1] for x in (together.tokens, together.lens, together.logprobs, together.no_speech_prob)], b)
    ctx.set_lanes(2)
    try:   # 17 rows on two lanes: two groups (9 + 8)
        rows = [i % 3 for i in range(17)]
        many = _aligned(ctx, mel3, _base(17), [prompts[i] for i in rows], n_frames=[nf[i] for i in rows], sot_tail=3)
    finally:
        ctx.set_lanes(0)
    for k, i in enumerate(rows):
        assert np.array_equal(many.start_frames[k], together.start_frames[i]), k
        assert np.array_equal(many.tokens[k], together.tokens[i]) and np.array_equal(_bits(many.logprobs[k]), _bits(together.logprobs[i]))
    with ctx.encode_windows(mel3, _base(3), 3000, 0, nf) as ws:
        from_set = ctx.transcribe_windows_aligned(ws, None, prompts, NEW, eot=EOT, seed=77, no_speech_token=NS_TOK, sot_tail=3)
        back = ctx.transcribe_windows_aligned(ws, [2, 0], [prompts[2], prompts[0]], NEW, eot=EOT, seed=77, no_speech_token=NS_TOK,
                                              sot_tail=3)
    assert np.array_equal(from_set.start_frames, together.start_frames)
    _same_decode(from_set, (together.tokens, together.lens, together.logprobs, together.no_speech_prob), "windows")
    assert np.array_equal(back.start_frames, together.start_frames[[2, 0]])


# ---------------------------------------------------------------- 5. degenerate rows
def test_degenerate_rows(dbg, pkg, mel3):
    _, _, ctx = dbg
    b = pkg.binding
    prompts = np.array([SOT_SEQ] * 3, dtype=np.int32)
    # A budget of 0 -- the one way to a row without a generated token -- is refused by wm_set_token_budgets as it always was
    # (budgets are >= 1), so len_b == 0 cannot reach the call; the smallest budget ends the row behind its first token.
    with pytest.raises(b.WhisperError) as e:
        _aligned(ctx, mel3, _base(3), prompts, budgets=[0, 24, 3])
    assert e.value.status == WM_ERR_INVALID
    r = _aligned(ctx, mel3, _base(3), prompts, budgets=[1, 24, 3])
    _same_decode(r, _plain(ctx, b, mel3, _base(3), prompts, budgets=[1, 24, 3]), "budget 1")
    assert int(r.lens[0]) == 1 and r.start_frames[0, 0] >= 0 and r.start_frames[0, 1] == 1500 and np.all(r.start_frames[0, 2:] == -1)
    assert int(r.lens[2]) == 3 and r.start_frames[2, 3] == 1500 and np.all(r.start_frames[2, 4:] == -1)
    # one generated token behind a prompt that ENDS in <|startoftranscript|>: one decoder row, nothing to z-score against
    r = _aligned(ctx, mel3, _base(3), prompts, n_frames=[3000, 1234, 3000], sot_index=2, budgets=[1, 1, 2])
    for k, M in ((0, 1500), (1, 617)):
        assert int(r.lens[k]) == 1 and r.start_frames[k].tolist() == [0, M] + [-1] * (NEW - 1), k
    assert int(r.lens[2]) == 2 and r.start_frames[2, 2] == 1500 and np.all(r.start_frames[2, :2] >= 0)    # two rows: aligned
    # a window of one frame decodes normally and has no audio frame to align to
    nf = [1, 3000, 1]
    r = _aligned(ctx, mel3, _base(3), prompts, n_frames=nf)
    _same_decode(r, _plain(ctx, b, mel3, _base(3), prompts, n_frames=nf), "one frame")
    assert int(r.lens[0]) >= 1 and np.all(r.start_frames[0] == -1) and np.all(r.start_frames[2] == -1)
    assert r.start_frames[1, int(r.lens[1])] == 1500


# ---------------------------------------------------------------- 6. invalid arguments
def test_invalid_arguments_and_the_context_still_works(dbg, pkg, mel3):
    _, _, ctx = dbg
    b = pkg.binding
    prompts = np.array([SOT_SEQ] * 3, dtype=np.int32)
    ragged = _ragged_prompts()
    good = _aligned(ctx, mel3, _base(3), prompts)
    bad = [dict(medfilt_width=6), dict(medfilt_width=0), dict(medfilt_width=-1), dict(medfilt_width=33),
           dict(qk_scale=float("nan")), dict(qk_scale=float("inf")),
           dict(prompts=ragged, sot_tail=0), dict(prompts=ragged, sot_tail=4),           # outside [1, the shortest prompt]
           dict(new=0), dict(new=446), dict(prompts=np.array([[10, 21, 1024]] * 3)),      # what the underlying call rejects
           dict(n_frames=3001), dict(sot_index=3), dict(T=-1.0), dict(budgets=[1, 2])]
    for kw in bad:
        a = dict(prompts=prompts)
        a.update(kw)
        with pytest.raises(b.WhisperError) as e:
            _aligned(ctx, mel3, _base(3), a.pop("prompts"), **a)
        assert e.value.status == WM_ERR_INVALID and str(e.value), kw
    # a null start_frame_out, through the raw symbol
    base, full, zero = _base(3), np.full(3, 3000, np.int32), np.zeros(3, np.int32)
    toks, lens, start = np.zeros((3, NEW), np.int32), np.zeros(3, np.int32), np.zeros((3, NEW + 1), np.int32)
    args = [b._ptr(mel3), b._ptr(base), b._ptr(full), b._ptr(zero), b._ptr(full), 3, b._ptr(prompts), 3, None, 0, None, NEW, EOT,
            None, 7, 1.0, b._ptr(toks), b._ptr(lens), None, None, b._ptr(start), b.WM_MEM_HOST]
    assert ctx.lib.wm_transcribe_mel_aligned(ctx.handle, *args) == 0
    assert np.array_equal(toks, good.tokens) and np.array_equal(start, good.start_frames)     # (no opts, no extra outputs)
    null = list(args)
    null[20] = None
    assert ctx.lib.wm_transcribe_mel_aligned(ctx.handle, *null) == WM_ERR_INVALID and b"start_frame_out" in ctx.lib.wm_last_error()
    # the all-f32 debug precision path
    ctx.set_precision(True)
    try:
        with pytest.raises(b.WhisperError) as e:
            _aligned(ctx, mel3, _base(3), prompts)
        assert e.value.status == WM_ERR_STATE
    finally:
        ctx.set_precision(False)
    again = _aligned(ctx, mel3, _base(3), prompts)
    assert np.array_equal(again.start_frames, good.start_frames) and np.array_equal(again.tokens, good.tokens)


# ---------------------------------------------------------------- 7. transcribe_long(word_timestamps="decode")
class _Logged:
    """a context that notes the name of every method looked up on it"""

    def __init__(self, ctx):
        self._ctx, self.names = ctx, []

    def __getattr__(self, name):
        v = getattr(self._ctx, name)
        if callable(v):
            self.names.append(name)
        return v


def test_transcribe_long_words_from_the_decode(prod, pkg, prod_vocab):
    B = pkg.binding
    recs = _long_recs()[:2]
    kw = _kw(vocab=prod_vocab, word_timestamps="decode", temperatures=(0.0,))
    log = _Logged(prod)
    got = B.transcribe_long(log, recs, recording_ids=[7, 300], **kw)
    assert not [n for n in log.names if n.startswith("align")], log.names
    assert "transcribe_mel_aligned" in log.names and "transcribe_mel" not in log.names
    log2 = _Logged(prod)
    again = B.transcribe_long(log2, recs, recording_ids=[7, 300], reuse_encoder=True, **kw)
    assert again == got                                             # equal in every field
    assert not [n for n in log2.names if n.startswith("align")] and "transcribe_windows_aligned" in log2.names
    n_words = 0
    for o, x in zip(got, recs):
        mel = prod.logmel_long([x])[0]
        lang = B.Whisper.LANGUAGES[o["language"] - SOT - 1]
        last_speech = 0.0
        for w in o["windows"]:
            seek, size = w["seek"], w["segment_size"]
            mine = [s for s in o["segments"] if s["seek"] == seek]
            if w["skipped"]:
                assert mine == []
                continue
            r = prod.transcribe_mel_aligned(mel, [0], mel.shape[1], seek, size, [w["prompt"]], 32, eot=EOT2, no_speech_token=NS)
            n = int(r.lens[0])
            assert [int(t) for t in r.tokens[0, :n] if t != EOT2] == w["tokens"]
            result = {k: mine[0][k] if mine else 0.0 for k in ("temperature", "avg_logprob", "compression_ratio", "no_speech_prob")}
            segs, _, _ = B.window_segments(w["tokens"], seek, size, TSB, EOT2, result, prod_vocab, cleanup=False)
            text = [t for s in segs for t in s["tokens"] if t < EOT2]
            if text and size >= 2:
                toks, sf, pr = B.decode_alignment_text(r.tokens[0], n, r.start_frames[0], r.logprobs[0], EOT2, n_text=len(text))
                assert toks == text
                B.window_word_timestamps(prod_vocab, segs, sf, pr, seek, EOT2, last_speech, lang)
                ends = [s["words"][-1]["end"] for s in segs if s["words"]]
                if ends:
                    last_speech = ends[-1]
            else:
                for s in segs:
                    s["words"] = []
            B.clear_empty_segments(segs, EOT2, prod_vocab, words=True)
            assert len(mine) == len(segs)
            for s, m in zip(segs, mine):
                n_words += len(s["words"])
                assert (m["start"], m["end"], m["words"], m["tokens"]) == (s["start"], s["end"], s["words"], s["tokens"]), seek
                for wd in s["words"]:
                    assert wd["start"] <= wd["end"] and 0.0 <= wd["probability"] <= 1.0
    assert n_words > 0
