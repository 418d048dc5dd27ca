"""GPU tests of long-form word timestamps: wm_align_mel (wm_align on log-mel windows with one start sequence per row)
through the C ABI, and binding.transcribe_long(word_timestamps=True) on top.  Oracle and restatements: the fp32 decoder
forward and the numpy find_alignment of tests/test_align_gpu.py / test_align_cpu.py, the add_word_timestamps restatement of
tests/test_longform_words_cpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from test_align_cpu import _bytes_to_unicode, alignment_matrix, start_frames
from test_align_gpu import EOT, GATE_TINY, NO_TS, SOT_SEQ, _text, dbg, default_heads, oracle_forward  # noqa: F401  (dbg: fixture)
from test_longform_gpu import EOT2, SOT, TASK, TSB, _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_cpu import BRANCHES, ref_window_words
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    out = os.environ.get("WM_MEASURED_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "align_mel_measured.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


def _on_device(ctx, flat, fn):
    d = ctx.to_device(flat)
    try:
        return fn(d)
    finally:
        ctx.dev_free(d)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 1. equals wm_align
@pytest.mark.parametrize("Bn", [1, 9, 130])
def test_full_windows_equal_wm_align_bit_for_bit(lively, pkg, Bn):
    _, _, _, ctx = lively
    b = pkg.binding
    rng = np.random.default_rng(Bn)
    pcm = np.concatenate([tones(13)] * 10)[:Bn]
    lens = [int(v) for v in rng.integers(0, 13, size=Bn)]
    lens[0] = 12
    if Bn > 4:
        lens[4], lens[Bn - 1] = 0, 7
    texts = [_text(rng, n) for n in lens]
    want = ctx.align(pcm, texts, SOT_SEQ, NO_TS, EOT)
    assert Bn <= 4 or (np.all(want[0][4] == -1) and np.all(want[1][4] == 0))
    mel = np.concatenate([ctx.logmel(pcm[i:i + 13], out_dtype=np.float32) for i in range(0, Bn, 13)])
    base = np.arange(Bn, dtype=np.int64) * 80 * 3000
    _same(ctx.align_mel(mel, base, 3000, 0, 3000, texts, SOT_SEQ, NO_TS, EOT), want)
    _same(_on_device(ctx, mel, lambda d: ctx.align_mel(d, base, 3000, 0, 3000, texts, SOT_SEQ, NO_TS, EOT,
                                                       mem=b.WM_MEM_DEVICE)), want)


# ---------------------------------------------------------------- 2. a window equals its materialised copy
def _recordings_mel(ctx):
    recs = [tones(1, i)[0][: 480000 - 70000 * i] for i in range(3)] + [np.concatenate([tones(1, 5)[0], tones(1, 6)[0]])]
    mels = ctx.logmel_long(recs)
    flat = np.concatenate([m.reshape(-1) for m in mels])
    base = np.cumsum([0] + [m.size for m in mels[:-1]]).astype(np.int64)
    return mels, flat, base, np.array([m.shape[1] for m in mels], dtype=np.int32)


#        (recording, seek, n_frames); -1: the window ends at the recording's last frame
WINDOWS = [(0, 0, 3000), (1, 777, 2), (2, 1501, 3), (3, 4001, 1233), (3, 2, 2999), (0, -1, 3000), (1, -1, 601), (2, 3333, 14),
           (3, 6000, 3000)]


def _window_rows(mels, base, Ts):
    rec = [w[0] for w in WINDOWS]
    nf = np.array([w[2] for w in WINDOWS], dtype=np.int32)
    seek = np.array([int(Ts[r]) - n if s < 0 else s for r, s, n in WINDOWS], dtype=np.int32)
    assert all(seek[i] + nf[i] <= Ts[rec[i]] for i in range(len(rec))) and any(seek[i] + nf[i] == Ts[rec[i]] for i in range(len(rec)))
    return rec, seek, nf


def test_a_window_equals_its_materialised_copy(lively, pkg):
    _, _, _, ctx = lively
    b = pkg.binding
    rng = np.random.default_rng(2)
    mels, flat, base, Ts = _recordings_mel(ctx)
    rec, seek, nf = _window_rows(mels, base, Ts)
    texts = [_text(rng, int(n)) for n in rng.integers(1, 13, size=len(rec))]
    got = ctx.align_mel(flat, base[rec], Ts[rec], seek, nf, texts, SOT_SEQ, NO_TS, EOT)
    got_d = _on_device(ctx, flat, lambda d: ctx.align_mel(d, base[rec], Ts[rec], seek, nf, texts, SOT_SEQ, NO_TS, EOT,
                                                          mem=b.WM_MEM_DEVICE))
    _same(got_d, got)
    for i, r in enumerate(rec):
        n = len(texts[i])
        block = np.ascontiguousarray(mels[r][:, seek[i]:seek[i] + nf[i]])       # its own [n_mels][n_frames] block
        one = ctx.align_mel(block, [0], int(nf[i]), 0, int(nf[i]), [texts[i]], SOT_SEQ, NO_TS, EOT)
        assert np.array_equal(one[0][0, :n + 1], got[0][i, :n + 1]) and np.array_equal(one[1][0, :n], got[1][i, :n]), WINDOWS[i]
        assert np.all(got[0][i, n + 1:] == -1)
        if nf[i] >= 4:   # (one audio frame: the z-score over identical softmax values is 0 / 0, as in openai-whisper)
            assert np.all(got[0][i, :n + 1] >= 0) and got[0][i, n] <= nf[i] // 2 - 1


# ---------------------------------------------------------------- 3. per-row start sequences
def test_per_row_start_sequences_equal_each_row_alone(lively):
    _, _, _, ctx = lively
    rng = np.random.default_rng(3)
    mel = ctx.logmel(tones(5), out_dtype=np.float32)
    base = np.arange(5, dtype=np.int64) * 240000
    sots = [[10, 21 + r, 5] for r in range(5)]
    texts = [_text(rng, n) for n in (7, 0, 12, 3, 9)]
    nf = [3000, 1500, 2001, 600, 3000]
    got = ctx.align_mel(mel, base, 3000, 0, nf, texts, sots, NO_TS, EOT)
    shared = ctx.align_mel(mel, base, 3000, 0, nf, texts, sots[0], NO_TS, EOT)
    assert not np.array_equal(got[1][2], shared[1][2])      # the start sequence matters
    _same([x[:1] for x in got], [x[:1] for x in shared])
    for r in range(5):
        n = len(texts[r])
        one = ctx.align_mel(mel, base[r:r + 1], 3000, 0, nf[r], [texts[r]], [sots[r]], NO_TS, EOT)
        assert np.array_equal(one[0][0, :n + 1], got[0][r, :n + 1]) and np.array_equal(one[1][0, :n], got[1][r, :n]), r
    # across decode groups: 130 rows, each with its own start sequence; rows 0, 64, 129 alone
    big = 130
    idx = [i % 5 for i in range(big)]
    sots_b = [[10, 21 + (i % 40), 5] for i in range(big)]
    texts_b = [_text(rng, 1 + i % 6) for i in range(big)]
    got_b = ctx.align_mel(mel, base[idx], 3000, 0, 3000, texts_b, sots_b, NO_TS, EOT)
    for r in (0, 64, 129):
        n = len(texts_b[r])
        one = ctx.align_mel(mel, base[idx[r]:idx[r] + 1], 3000, 0, 3000, [texts_b[r]], [sots_b[r]], NO_TS, EOT)
        assert np.array_equal(one[0][0, :n + 1], got_b[0][r, :n + 1]) and np.array_equal(one[1][0, :n], got_b[1][r, :n]), r


# ---------------------------------------------------------------- 4. against the fp32 oracle on seek windows
# Windows inside and at the end of recordings of different lengths, full and short.  The frame counts stay at 200 and
# above: what a seek window changes against wm_align is the encoder's input (another normalisation, another position, the
# zero padding), which these cover; the filter's edge cases (a handful of frames) are a property of the alignment kernels,
# covered for wm_align by test_align_gpu.py and tied to this entry point bit for bit by the 2-, 3- and 14-frame windows of
# test_a_window_equals_its_materialised_copy.
ORACLE_WINDOWS = [("default", 0, 0, 3000, 7), ("explicit", 1, 777, 1234, 7), ("default", 3, 4001, 2999, 1),
                  ("explicit", 2, -1, 601, 7), ("default", 3, 6100, 200, 7)]


@pytest.mark.parametrize("heads, rec, seek, n_frames, width", ORACLE_WINDOWS)
def test_seek_windows_against_the_oracle(dbg, heads, rec, seek, n_frames, width):
    """Measured on an MI355X (cost-matrix rel-L2 against the fp32 restatement, gate GATE_TINY = 0.06): see
    profiles/r10_longform_words.txt."""
    dims, sd, ctx = dbg
    rng = np.random.default_rng(seek + n_frames)
    mels, flat, base, Ts = _recordings_mel(ctx)
    if seek < 0:
        seek = int(Ts[rec]) - n_frames
    hl = default_heads(dims) if heads == "default" else [(0, 1), (1, 0)]
    ctx.set_alignment_heads([] if heads == "default" else hl)
    try:
        texts = [_text(rng, 23), _text(rng, 5), _text(rng, 1)]
        sots = [SOT_SEQ, [10, 22, 5], [11, 21, 5]]
        sf, pr, mat = ctx.align_mel(flat, base[[rec] * 3], Ts[[rec] * 3], seek, n_frames, texts, sots, NO_TS, EOT,
                                    medfilt_width=width, capture_matrix=True)
    finally:
        ctx.set_alignment_heads([])
    win = np.zeros((1, 80, 3000), dtype=np.float32)
    win[0, :, :n_frames] = mels[rec][:, seek:seek + n_frames]
    xa = ctx.encode_mel(win)
    S, M = 3, n_frames // 2
    key = "window_%d_%d_%d" % (rec, seek, n_frames)
    for b, t in enumerate(texts):
        n = len(t)
        seq = sots[b] + [NO_TS] + t + [EOT]
        logits, qk = oracle_forward(sd, dims, seq, xa[0])
        want = alignment_matrix(np.stack([qk[l, h] for l, h in hl]), S, n_frames, width, 1.0)
        got = mat[b, :n + 1, :M]
        assert np.all(mat[b, n + 1:] == 0) and np.all(mat[b, :, M:] == 0)
        e = R.rel_l2(got, want)
        _note(key + "_rel_l2", e)
        print("align_mel oracle %s row %d: rel-L2 %.5f (gate %.3f)" % (key, b, e, GATE_TINY))
        assert e <= GATE_TINY, (key, b, e)
        own = start_frames(got)     # DTW: bit-exact against numpy f32 on the GPU's own matrix
        assert sf[b, :n + 1].tolist() == own.tolist(), (key, b)
        assert np.all(sf[b, n + 1:] == -1)
        d = np.abs(start_frames(want) - own)
        _note(key + "_frame_median", np.median(d))
        _note(key + "_frame_max", d.max())
        assert np.median(d) <= 1, (key, b, d)
        own_l = ctx.decode_logits(np.asarray([seq[:-1]], dtype=np.int32), xa)[0]
        p_own = torch.softmax(torch.as_tensor(own_l[S:S + n, :EOT]).double(), -1).numpy()[np.arange(n), t]
        p_ref = torch.softmax(torch.as_tensor(logits[S:S + n, :EOT]).double(), -1).numpy()[np.arange(n), t]
        d_own = np.abs(pr[b, :n] - p_own).max()
        _note(key + "_prob_own", d_own)
        assert d_own <= 1e-5 + 1e-4 * p_own.max(), (key, b, d_own)
        d_ref = np.abs(pr[b, :n] - p_ref).max()
        _note(key + "_prob_oracle", d_ref)
        assert d_ref <= 2e-3, (key, b, d_ref)
        assert np.all(pr[b, n:] == 0)


# ---------------------------------------------------------------- 5. invalid arguments
def test_invalid_align_mel_arguments(lively, pkg):
    dims, _, _, ctx = lively
    b = pkg.binding
    mel = np.zeros((2, 80, 3000), np.float32)
    base = np.array([0, 240000], np.int64)
    ok = dict(mel_len=3000, seek=0, n_frames=3000, texts=[[1, 2, 3], [4]], sots=[SOT_SEQ, SOT_SEQ], no_ts=NO_TS, eot=EOT,
              medfilt_width=7, qk_scale=1.0, base=base)

    def call(**kw):
        a = dict(ok, **kw)
        return ctx.align_mel(mel, a["base"], a["mel_len"], a["seek"], a["n_frames"], a["texts"], a["sots"], a["no_ts"],
                             a["eot"], medfilt_width=a["medfilt_width"], qk_scale=a["qk_scale"])
    bad = [dict(texts=[[1], [EOT]]), dict(texts=[[-1], [1]]), dict(texts=[[1] * 444, [1]]),           # what wm_align rejects
           dict(n_frames=[3000, 1]), dict(n_frames=[3001, 3000]), dict(medfilt_width=6), dict(medfilt_width=0),
           dict(medfilt_width=-3), dict(medfilt_width=33), dict(qk_scale=float("nan")), dict(qk_scale=float("inf")),
           dict(no_ts=dims["n_vocab"]), dict(eot=-1),
           dict(mel_len=[3000, 0]), dict(seek=[0, -1]), dict(seek=[0, 1]), dict(n_frames=[3000, 2], seek=[0, 2999]),   # a window
           dict(base=np.array([0, -5], np.int64)), dict(n_frames=[0, 3000]),
           dict(sots=[SOT_SEQ, [10, dims["n_vocab"], 5]]), dict(sots=[[-1, 21, 5], SOT_SEQ])]       # a start-sequence token
    for kw in bad:
        with pytest.raises(b.WhisperError) as e:
            call(**kw)
        assert e.value.status == WM_ERR_INVALID and str(e.value), kw
    # null pointers, through the raw symbol
    i32, out_i, i64, f32 = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(2, np.int64), np.zeros(16, np.float32)
    full, sot, text, one = np.full(2, 3000, np.int32), np.array(SOT_SEQ, np.int32), np.ones(4, np.int32), np.ones(1, np.int32)
    good = [b._ptr(mel), b._ptr(i64), b._ptr(full), b._ptr(i32), b._ptr(full), 1, b._ptr(sot), 3, NO_TS, EOT, b._ptr(text),
            b._ptr(one), 4, 7, 1.0, b._ptr(out_i), b._ptr(f32), b.WM_MEM_HOST]
    for k in (0, 1, 2, 3, 4, 6, 10, 11, 15):
        args = list(good)
        args[k] = None
        assert ctx.lib.wm_align_mel(ctx.handle, *args) == WM_ERR_INVALID, k
        assert b"null" in ctx.lib.wm_last_error()
    assert ctx.lib.wm_align_mel(ctx.handle, *(good[:5] + [0] + good[6:])) == WM_ERR_INVALID      # B < 1
    # a valid call goes through afterwards; token_prob_out is optional
    sf, pr = call()
    assert np.all(sf[0, :4] >= 0) and np.all(sf[1, :2] >= 0) and np.all(sf[1, 2:] == -1)
    args = list(good)
    args[16] = None
    assert ctx.lib.wm_align_mel(ctx.handle, *args) == 0 and out_i[0] >= 0 and out_i[2] == -1
    sf, pr = call(texts=[[1] * 443, [2]])      # 3 + 443 + 2 = 448: the longest allowed
    assert sf.shape == (2, 444) and np.all(np.diff(sf[0]) >= 0)


# ---------------------------------------------------------------- 6. decode is untouched
def test_greedy_is_unchanged_around_align_mel(lively):
    _, _, _, ctx = lively
    pcm = tones(3)
    t0, l0 = ctx.transcribe_greedy(pcm, SOT_SEQ, 20, eot=EOT)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    texts = [list(t0[b, :max(int(l0[b]) - 1, 0)]) for b in range(3)]
    ctx.align_mel(mel, np.arange(3, dtype=np.int64) * 240000, 3000, [0, 5, 1000], [3000, 2995, 777], texts,
                  [[10, 21 + b, 5] for b in range(3)], NO_TS, EOT)
    t1, l1 = ctx.transcribe_greedy(pcm, SOT_SEQ, 20, eot=EOT)
    assert np.array_equal(t0, t1) and np.array_equal(l0, l1)


# ---------------------------------------------------------------- 7. transcribe_long(word_timestamps=True)
NO_TS2 = 50363


def _piece(i):
    return (" w%d" % i) if i % 3 else ("x%d" % i)


@pytest.fixture(scope="module")
def prod_vocab(pkg, tmp_path_factory):
    b2u = _bytes_to_unicode()
    path = tmp_path_factory.mktemp("vocab") / "vocab.json"
    path.write_text(json.dumps({"".join(b2u[c] for c in _piece(i).encode()): i for i in range(EOT2)}))
    v = pkg.binding.Vocab(str(path))
    yield v
    v.close()


def _strip_words(o):
    return (o["language"], o["seeks"], [(w["seek"], w["segment_size"], w["temperatures"], w["skipped"], w["tokens"])
                                        for w in o["windows"]], o["segments"])


def _words_kw(vocab, **extra):
    return _kw(vocab=vocab, word_timestamps=True, no_timestamps=NO_TS2, **extra)


def test_transcribe_long_word_timestamps(prod, pkg, prod_vocab):
    B = pkg.binding
    recs = _long_recs()
    ids = [7, 300, 65535, 0]
    got = prod.transcribe_long(recs, recording_ids=ids, **_words_kw(prod_vocab))
    for r, x in enumerate(recs):
        alone = prod.transcribe_long([x], recording_ids=[ids[r]], **_words_kw(prod_vocab))[0]
        assert _strip_words(alone) == _strip_words(got[r]), "recording %d" % r
    by_word_end = by_timestamp = n_words = 0
    count = dict.fromkeys(BRANCHES, 0)
    dummy = dict(temperature=0.0, avg_logprob=0.0, compression_ratio=1.0, no_speech_prob=0.0)
    for o, x in zip(got, recs):
        mel = prod.logmel_long([x])[0]
        content = mel.shape[1] - 3000
        lang = B.Whisper.LANGUAGES[o["language"] - SOT - 1]
        last_speech = 0.0
        for k, w in enumerate(o["windows"]):
            seek, size = w["seek"], w["segment_size"]
            assert size == min(3000, content - seek)
            mine = [s for s in o["segments"] if s["seek"] == seek]
            if w["skipped"]:
                want_seek = seek + size
                assert mine == []
            else:
                segs, want_seek, single = B.window_segments(w["tokens"], seek, size, TSB, EOT2, dummy, prod_vocab, cleanup=False)
                text = [t for s in segs for t in s["tokens"] if t < EOT2]
                if text and size >= 2:
                    sf, pr = prod.align_mel(mel, [0], mel.shape[1], seek, size, [text], [[SOT, o["language"], TASK]], NO_TS2,
                                            EOT2)
                    last_speech = ref_window_words(segs, [int(v) for v in sf[0]], list(pr[0]), seek, last_speech, lang, count,
                                                   piece=_piece, eot=EOT2)
                    ends = [s["words"][-1]["end"] for s in segs if s["words"]]
                    if ends:
                        if not single and ends[-1] > seek / 100:
                            want_seek = round(ends[-1] * 100)
                            by_word_end += 1
                        else:
                            by_timestamp += 1
                        last_speech = ends[-1]
                    else:
                        by_timestamp += 1
                else:
                    for s in segs:
                        s["words"] = []
                    by_timestamp += 1
                assert len(mine) == len(segs)
                for s, m in zip(segs, mine):
                    for wd in s["words"]:
                        n_words += 1
                        assert wd["start"] <= wd["end"], (seek, wd)
                        assert max(0.0, seek / 100 - 1.4) <= wd["start"] and wd["end"] <= seek / 100 + 30.7, (seek, wd)
                        assert 0.0 <= wd["probability"] <= 1.0
                    if s["start"] == s["end"] or s["text"].strip() == "":      # the clean-up, after the word step
                        s["words"], s["tokens"] = [], []
                    assert (m["start"], m["end"], m["words"], m["tokens"]) == (s["start"], s["end"], s["words"], s["tokens"]), seek
            if k + 1 < len(o["windows"]):
                assert o["windows"][k + 1]["seek"] == want_seek, (seek, want_seek)
            else:
                assert want_seek >= content
    print("long-form words: %d words, %d windows moved the seek by the last word end, %d by the timestamp rule; branches %s"
          % (n_words, by_word_end, by_timestamp, count))
    assert n_words > 0 and by_word_end >= 1 and by_timestamp >= 1


def test_transcribe_long_word_timestamps_with_conditioning(prod, prod_vocab):
    from test_longform_gpu import SOT_PREV
    recs = _long_recs()[:3]
    kw = _words_kw(prod_vocab, condition_on_previous_text=True, sot_prev=SOT_PREV)
    got = prod.transcribe_long(recs, recording_ids=[3, 2, 9], **kw)
    assert any(s.get("words") for o in got for s in o["segments"])
    for r, x in enumerate(recs):
        alone = prod.transcribe_long([x], recording_ids=[[3, 2, 9][r]], **kw)[0]
        assert _strip_words(alone) == _strip_words(got[r]), "recording %d" % r
