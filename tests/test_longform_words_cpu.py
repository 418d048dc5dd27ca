"""CPU tests of long-form word timestamps: binding.window_word_timestamps (openai-whisper's add_word_timestamps for one
window) against an independent restatement written here, the word step of binding.transcribe_long's rounds on a fake
decode / align pair, and the wm_align_mel export.  The rules restated (times in seconds, one alignment frame = 0.02 s):

  1. the window's text tokens are the tokens < eot of its segments, concatenated;
  2. words before punctuation merging: the tokens plus a final <|endoftext|> split per token for zh / ja / th / lo / my / yue
     and at spaces / ASCII punctuation otherwise; a word of tokens [a, b) spans [start_frames[a], start_frames[b]) / 50, its
     probability is the mean of its tokens'; the last word (<|endoftext|>) is dropped;
  3. median = min(0.7, median of the non-zero word durations), 0 without any; max_duration = 2 * median;
  4. with a non-zero duration: from the second word on, a word longer than max_duration that is a sentence-end mark is cut
     to start + max_duration, else one that follows a sentence-end mark to end - max_duration;
  5. merge_punctuations;  6. the words are dealt to the segments by their token counts, non-empty ones kept, times rounded
     to 0.01 behind the window's offset;  7. the first-word pause rule, segment start / end against first / last word;
  8. every segment gets `words`.
"""
import ctypes
import importlib
import json
import os
import string

import numpy as np
import pytest

from conftest import GOLDEN
from test_align_cpu import _bytes_to_unicode

B = importlib.import_module("openai_whisper_coreml_amd.binding")

# ids of the test vocabulary (all pieces are whole UTF-8 characters, so a per-token split is the unicode split)
PIECES = [" a", " b", " c", ".", ",", " (", ")", "?", "中", "文", "。", " d", "e", "!", " f ", " \""]
EOT, TB = 50, 100
MARKS = ".。!！?？"
PRE, APP = "\"'“¿([{-", "\"'.。,，!！?？:：”)]}、"
NO_SPACE = ("zh", "ja", "th", "lo", "my", "yue")
BRANCHES = ("r4_end", "r4_start", "r7a_boundary", "r7a_plain", "r7b_word", "r7b_segment", "r7c_word", "r7c_segment")


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    b2u = _bytes_to_unicode()
    path = tmp_path_factory.mktemp("vocab") / "vocab.json"
    path.write_text(json.dumps({"".join(b2u[c] for c in p.encode()): i for i, p in enumerate(PIECES)}), encoding="utf-8")
    v = B.Vocab(str(path))
    yield v
    v.close()


# ---------------------------------------------------------------- the restatement
def ref_window_words(segments, start_frames, token_probs, seek, last_speech, language, count, piece=None, eot=EOT):
    """Rules 1-8 on plain lists; `segments` are edited in place.  count: dict of branch counters; piece(id): the text of a
    token (every piece a whole number of UTF-8 characters), default the test vocabulary's."""
    piece = piece or (lambda t: PIECES[t])
    per_seg = [[t for t in s["tokens"] if t < eot] for s in segments]
    toks = [t for ts in per_seg for t in ts]
    # 2. words: (text, token count)
    groups = []
    for t in toks:
        p = piece(t)
        if language in NO_SPACE or not groups or p.startswith(" ") or p.strip() in string.punctuation:
            groups.append([p, 1])
        else:
            groups[-1][0] += p
            groups[-1][1] += 1
    words, a = [], 0
    for text, n in groups:
        words.append(dict(word=text, n=n, start=start_frames[a] / 50, end=start_frames[a + n] / 50,
                          probability=float(np.mean(np.asarray(token_probs[a:a + n], dtype=np.float64)))))
        a += n
    # 3.
    dur = sorted(w["end"] - w["start"] for w in words if w["end"] - w["start"] != 0)
    if dur:
        k = len(dur)
        med = dur[k // 2] if k % 2 else (dur[k // 2 - 1] + dur[k // 2]) / 2
        median = min(0.7, med)
    else:
        median = 0.0
    max_duration = 2 * median
    # 4.
    if dur:
        for i in range(1, len(words)):
            w = words[i]
            if w["end"] - w["start"] > max_duration:
                if w["word"] in list(MARKS):
                    w["end"] = w["start"] + max_duration
                    count["r4_end"] += 1
                elif words[i - 1]["word"] in list(MARKS):
                    w["start"] = w["end"] - max_duration
                    count["r4_start"] += 1
    # 5. prepended marks travel forward into the next word, appended marks back into the previous one
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i]["word"].startswith(" ") and words[i]["word"].strip() in PRE:
            words[j]["word"] = words[i]["word"] + words[j]["word"]
            words[j]["n"] += words[i]["n"]
            words[i]["word"], words[i]["n"] = "", 0
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i]["word"].endswith(" ") and words[j]["word"] in APP:
            words[i]["word"] += words[j]["word"]
            words[i]["n"] += words[j]["n"]
            words[j]["word"], words[j]["n"] = "", 0
        else:
            i = j
        j += 1
    # 6. - 8.
    off = seek / 100
    wi = 0
    for seg, ts in zip(segments, per_seg):
        taken, ws = 0, []
        while wi < len(words) and taken < len(ts):
            w = words[wi]
            if w["word"] != "":
                ws.append(dict(word=w["word"], start=round(off + w["start"], 2), end=round(off + w["end"], 2),
                               probability=w["probability"]))
            taken += w["n"]
            wi += 1
        if ws:
            two = len(ws) >= 2
            if ws[0]["end"] - last_speech > 4 * median and (
                    ws[0]["end"] - ws[0]["start"] > max_duration or (two and ws[1]["end"] - ws[0]["start"] > 2 * max_duration)):
                if two and ws[1]["end"] - ws[1]["start"] > max_duration:
                    boundary = max(ws[1]["end"] / 2, ws[1]["end"] - max_duration)
                    ws[0]["end"] = ws[1]["start"] = boundary
                    count["r7a_boundary"] += 1
                else:
                    count["r7a_plain"] += 1
                ws[0]["start"] = max(0, ws[0]["end"] - max_duration)
            if seg["start"] < ws[0]["end"] and seg["start"] - 0.5 > ws[0]["start"]:
                ws[0]["start"] = max(0, min(ws[0]["end"] - median, seg["start"]))
                count["r7b_word"] += 1
            else:
                seg["start"] = ws[0]["start"]
                count["r7b_segment"] += 1
            if seg["end"] > ws[-1]["start"] and seg["end"] + 0.5 < ws[-1]["end"]:
                ws[-1]["end"] = max(ws[-1]["start"] + median, seg["end"])
                count["r7c_word"] += 1
            else:
                seg["end"] = ws[-1]["end"]
                count["r7c_segment"] += 1
            last_speech = seg["end"]
        seg["words"] = ws
    return last_speech


def _segments(token_lists, times):
    return [dict(seek=0, start=float(s), end=float(e), tokens=list(t)) for t, (s, e) in zip(token_lists, times)]


def _both(vocab, token_lists, times, sf, pr, seek, last, language=None):
    """the implementation and the restatement on copies of the same window: (segments, last speech, branch counts)"""
    count = dict.fromkeys(BRANCHES, 0)
    got, want = _segments(token_lists, times), _segments(token_lists, times)
    last_got = B.window_word_timestamps(vocab, got, np.asarray(sf), np.asarray(pr, dtype=np.float32), seek, EOT, last,
                                        language, PRE, APP)
    last_want = ref_window_words(want, list(sf), list(np.asarray(pr, dtype=np.float32)), seek, last, language, count)
    assert got == want and last_got == last_want, (got, want)
    return got, last_got, count


def _only(count, *names):
    return all((count[k] > 0) == (k in names) for k in BRANCHES if k.startswith(("r4", "r7a")) or k in names)


# ---------------------------------------------------------------- hand-built cases, one branch each
def test_rule_4_a_long_sentence_end_mark_is_cut_at_its_start_side(vocab):
    # " f " (trailing space: "." is not merged into it), "." lasting 2 s among 0.2 s words: median 0.2, cut to 0.4
    toks = [[TB, 0, 14, 3, 1, TB + 200]]
    sf = [0, 10, 20, 120, 130, 130]
    segs, last, count = _both(vocab, toks, [(0.0, 4.0)], sf, [0.5] * 4, 0, 0.0)
    assert _only(count, "r4_end", "r7b_segment", "r7c_segment")
    assert [(w["word"], w["start"], w["end"]) for w in segs[0]["words"]] == [
        (" a", 0.0, 0.2), (" f ", 0.2, 0.4), (".", 0.4, 0.8), (" b", 2.4, 2.6)]
    assert segs[0]["start"] == 0.0 and segs[0]["end"] == 2.6 == last


def test_rule_4_a_long_word_behind_a_sentence_end_is_cut_at_its_end_side(vocab):
    toks = [[TB, 0, 14, 3, 1, 2, TB + 200]]
    sf = [0, 10, 20, 30, 130, 140, 140]
    segs, _, count = _both(vocab, toks, [(0.0, 4.0)], sf, [0.5] * 5, 0, 0.0)
    assert _only(count, "r4_start", "r7b_segment", "r7c_segment")
    assert [(w["word"], w["start"], w["end"]) for w in segs[0]["words"]][3] == (" b", 2.2, 2.6)


def test_rule_7a_long_first_word_after_a_pause(vocab):
    toks = [[TB, 0, 1, 2, 11, TB + 400]]
    sf = [100, 250, 260, 270, 280, 280]       # " a" lasts 3 s, the others 0.2: median 0.2
    segs, _, count = _both(vocab, toks, [(5.0, 13.0)], sf, [0.5] * 4, 300, 0.0)
    assert _only(count, "r7a_plain", "r7b_segment", "r7c_segment")
    assert (segs[0]["words"][0]["start"], segs[0]["words"][0]["end"]) == (8.0 - 0.4, 8.0) and segs[0]["start"] == 7.6
    # no pause in front of it (the last speech ended 0.5 s before the word's end): the word keeps its start
    segs, _, count = _both(vocab, toks, [(5.0, 13.0)], sf, [0.5] * 4, 300, 7.5)
    assert _only(count, "r7b_segment", "r7c_segment") and segs[0]["words"][0]["start"] == 5.0


def test_rule_7a_long_second_word_moves_the_boundary(vocab):
    toks = [[TB, 0, 1, 2, 11, 0, TB + 400]]
    sf = [100, 250, 325, 335, 345, 355, 355]  # " a" 3 s, " b" 1.5 s, three words of 0.2 s: median 0.2
    segs, _, count = _both(vocab, toks, [(2.0, 7.1)], sf, [0.5] * 5, 0, 0.0)
    assert _only(count, "r7a_boundary", "r7b_segment", "r7c_segment")
    w = segs[0]["words"]
    assert w[0]["end"] == w[1]["start"] == 6.5 - 0.4 and w[0]["start"] == 6.5 - 0.4 - 0.4 and w[1]["end"] == 6.5


def test_rule_7b_segment_start_inside_a_long_first_word(vocab):
    toks = [[TB + 150, 0, 1, 2, TB + 300]]
    sf = [50, 200, 210, 220, 220]             # " a" 1.0 .. 4.0 s; the segment's own timestamp says 3.0
    segs, _, count = _both(vocab, toks, [(3.0, 6.0)], sf, [0.5] * 3, 0, 4.0)
    assert _only(count, "r7b_word", "r7c_segment")
    assert segs[0]["words"][0]["start"] == 3.0 and segs[0]["start"] == 3.0 and segs[0]["end"] == 4.4
    # a median that leaves less than the segment's start: end - median wins
    sf = [50, 200, 280, 360, 360]
    segs, _, _ = _both(vocab, toks, [(3.8, 9.0)], sf, [0.5] * 3, 0, 4.0)
    assert segs[0]["words"][0]["start"] == 4.0 - 0.7 and segs[0]["start"] == 3.8


def test_rule_7c_segment_end_inside_a_long_last_word(vocab):
    toks = [[TB, 0, 1, 2, TB + 100]]
    sf = [0, 10, 20, 200, 200]                # " c" 0.4 .. 4.0 s; the segment's own timestamp says 2.0
    segs, last, count = _both(vocab, toks, [(0.0, 2.0)], sf, [0.5] * 3, 0, 0.0)
    assert _only(count, "r7b_segment", "r7c_word")
    assert segs[0]["words"][-1]["end"] == 2.0 and segs[0]["end"] == 2.0 == last


def test_words_are_dealt_to_the_segments_by_token_count(vocab):
    # " (" travels forward into " b" across the segment border and leaves a word without tokens behind, which does not
    # count towards the first segment's two tokens: that segment takes the merged word too (openai-whisper's running index)
    toks = [[TB, 0, 5, TB + 50], [TB + 50, 1, 6, 3, TB + 90], [TB + 90, TB + 95], [TB + 95, 8, 9, 10]]
    sf = [0, 10, 20, 30, 40, 50, 60, 70, 80]
    times = [(0.0, 1.0), (1.0, 1.8), (1.8, 1.9), (1.9, 30.0)]
    segs, last, _ = _both(vocab, toks, times, sf, np.linspace(0.1, 0.8, 8), 1000, 10.0, "zh")
    assert [[w["word"] for w in s["words"]] for s in segs] == [[" a", " ( b)."], ["中", "文。"], [], []]
    assert (segs[2]["start"], segs[2]["end"]) == (1.8, 1.9) and (segs[3]["start"], segs[3]["end"]) == (1.9, 30.0)  # untouched
    assert (segs[0]["words"][1]["start"], segs[0]["words"][1]["end"]) == (10.4, 10.6) and last == segs[1]["end"] == 11.4
    # the space rule on the same tokens: the CJK pieces continue the word in front of them
    segs, _, _ = _both(vocab, toks, times, sf, np.linspace(0.1, 0.8, 8), 1000, 10.0, "en")
    assert [w["word"] for s in segs for w in s["words"]] == [" a", " ( b)", ".中文。"]


def test_window_without_a_non_zero_duration(vocab):
    segs, last, count = _both(vocab, [[TB, 0, 1, TB + 5]], [(7.0, 7.1)], [30, 30, 30], [0.25, 0.75], 700, 3.0)
    assert [(w["start"], w["end"]) for w in segs[0]["words"]] == [(7.6, 7.6)] * 2
    assert (segs[0]["start"], segs[0]["end"], last) == (7.6, 7.6, 7.6) and _only(count, "r7b_segment", "r7c_segment")


# ---------------------------------------------------------------- random windows
def _random_window(rng):
    n_seg = int(rng.integers(1, 5))
    lists, n_text = [], []
    for _ in range(n_seg):
        n = int(rng.choice([0, 1, 2, 3, 5, 8], p=[0.1, 0.15, 0.2, 0.2, 0.2, 0.15]))
        body = [int(t) for t in rng.choice(len(PIECES), size=n, p=_PIECE_P)]
        lists.append([TB + int(rng.integers(0, 1500))] + body + ([TB + int(rng.integers(0, 1500))] if rng.random() < 0.8 else []))
        n_text.append(n)
    total = sum(n_text)
    step = rng.choice([0, 1, 2, 3], size=total + 1, p=[0.3, 0.45, 0.15, 0.1])
    inc = np.where(step == 0, 0, np.where(step == 1, rng.integers(1, 16, total + 1),
                                          np.where(step == 2, rng.integers(25, 60, total + 1),
                                                   rng.integers(60, 300, total + 1))))
    sf = np.minimum(np.cumsum(inc) + int(rng.integers(0, 200)), 1499)
    seek = int(rng.integers(0, 20000))
    times, a = [], 0
    for n in n_text:   # segment times near the segment's own tokens, so that rules 7b / 7c see both outcomes
        s = seek / 100 + sf[a] / 50 + float(rng.uniform(-1.0, 3.0))
        e = seek / 100 + sf[a + n] / 50 + float(rng.uniform(-3.0, 1.0))
        times.append((round(max(s, 0.0), 2), round(max(e, 0.0), 2)))
        a += n
    last = float(rng.choice([0.0, max(seek / 100 - float(rng.uniform(0, 3)), 0.0), seek / 100 + float(rng.uniform(0, 10))]))
    return lists, times, sf, rng.random(max(total, 1)).astype(np.float32)[:total], seek, last


_PIECE_P = np.array([3, 3, 3, 2, 1, 1, 1, 1, 1, 1, 1, 3, 2, 1, 2, 1], dtype=np.float64)
_PIECE_P /= _PIECE_P.sum()


def test_random_windows_match_the_restatement_and_take_every_branch(vocab):
    rng = np.random.default_rng(20)
    total = dict.fromkeys(BRANCHES, 0)
    n_words = zero_len = 0
    for k in range(600):
        lists, times, sf, pr, seek, last = _random_window(rng)
        segs, _, count = _both(vocab, lists, times, sf, pr, seek, last, "ja" if k % 3 == 0 else "en")
        for key in BRANCHES:
            total[key] += count[key]
        for s in segs:
            n_words += len(s["words"])
            zero_len += sum(w["start"] == w["end"] for w in s["words"])
    assert all(total[k] > 0 for k in BRANCHES), total
    assert n_words > 1000 and zero_len > 50


# ---------------------------------------------------------------- the rounds of transcribe_long on a fake context
SOT, LANG_EN, LANG_ZH, TASK, SOT_PREV, NS, NO_TS = 40, 41, 42, 45, 46, 47, 48


class FakeCtx:
    """Canned logmel_long, transcribe_mel and align_mel.  script[(recording id, window ordinal)] = (generated tokens
    without eot, start frames of the window's text tokens + 1); a window without an entry decodes to DEFAULT."""
    DEFAULT = ([TB, 0, 1, TB + 500], [0, 100, 200])

    def __init__(self, script, n_ctx=64):
        self.dims = dict(n_text_ctx=n_ctx, n_mels=80, n_vocab=128)
        self.script = script
        self.round_ids = None
        self.align_calls = []

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
        n = len(sample_ids)
        self.round_ids = [int(s) for s in sample_ids]
        self.round_base = [int(b) for b in mel_base]
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.full(n, 0.01, dtype=np.float32)
        for i, sid in enumerate(sample_ids):
            body = self.script.get((int(sid) & 0xFFFF, int(sid) >> 16), self.DEFAULT)[0]
            if body == "skip":
                body, ns[i] = [], 0.9
            body = list(body) + [eot]
            toks[i, :len(body)] = body
            lens[i] = len(body)
            lp[i, :len(body)] = -5.0 if ns[i] > 0.5 else -0.1
        return B.TranscribeResult(toks, lens, lp, ns, eot)

    def align_mel(self, mel, mel_base, mel_len, seek, n_frames, text_tokens, sot_seqs, no_timestamps, eot, medfilt_width=7,
                  qk_scale=1.0, capture_matrix=False, mem=0):
        self.align_calls.append(dict(base=[int(b) for b in mel_base], seek=[int(s) for s in seek],
                                     n_frames=[int(n) for n in n_frames], texts=[list(map(int, t)) for t in text_tokens],
                                     sot=[list(map(int, s)) for s in sot_seqs], no_timestamps=no_timestamps,
                                     medfilt_width=medfilt_width, qk_scale=qk_scale, mem=mem))
        width = max(len(t) for t in text_tokens)
        sf = np.full((len(text_tokens), width + 1), -1, dtype=np.int32)
        pr = np.zeros((len(text_tokens), width), dtype=np.float32)
        for i, (b, t) in enumerate(zip(mel_base, text_tokens)):
            sid = self.round_ids[self.round_base.index(int(b))]
            frames = self.script.get((sid & 0xFFFF, sid >> 16), self.DEFAULT)[1]
            assert len(frames) == len(t) + 1, (sid, frames, t)
            sf[i, :len(t) + 1] = frames
            pr[i, :len(t)] = 0.5
        return sf, pr


def _fake_kw(**extra):
    kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TB, no_speech_token=NS, language=LANG_EN, sot_prev=SOT_PREV,
              compression_ratio_threshold=None)
    kw.update(extra)
    return kw


SCRIPT = {
    # recording 0 (70 s).  window 0 ends in a single timestamp: the seek takes the whole window whatever the words say
    (0, 0): ([TB, 0, 1, TB + 500], [0, 100, 200]),
    # window 1: no single-timestamp ending, last word ends at 6.0 s of the window: the seek follows it, not <|10.00|>
    (0, 1): ([TB, 0, 1, TB + 500, TB + 500, 2], [250, 275, 300]),
    # window 2 (seek 3600): every token at frame 0, so the last word ends AT the window's offset: the timestamp rule stays
    (0, 2): ([TB, 0, 1, TB + 250, TB + 250, 2], [0, 0, 0]),
    # window 3: an instantaneous segment by its timestamps whose words give it a duration (kept), and one with a duration
    # whose words are all zero-length at one frame (start == end after the word step: cleared)
    (0, 3): ([TB + 5, 0, TB + 5, TB + 5, 1, 2, TB + 100], [10, 60, 60, 60]),
    # recording 1 (50 s, zh): a skipped window, then the default one
    (1, 0): ("skip", None),
}


def _run(vocab, word_timestamps, **extra):
    recs = [np.zeros(16000 * 70, np.float32), np.zeros(16000 * 50, np.float32), np.zeros(160, np.float32)]
    ctx = FakeCtx(SCRIPT)
    kw = _fake_kw(language=[LANG_EN, LANG_ZH, LANG_EN], vocab=vocab, **extra)
    if word_timestamps:
        kw.update(word_timestamps=True, no_timestamps=NO_TS)
    return ctx, B.transcribe_long(ctx, recs, **kw)


def test_word_timestamps_off_returns_what_the_parent_returned(vocab):
    """tests/golden/longform_words_fake_parent.json: transcribe_long of the commit before word timestamps, on this fake"""
    ctx, out = _run(vocab, False)
    assert not ctx.align_calls
    with open(os.path.join(GOLDEN, "longform_words_fake_parent.json")) as f:
        want = json.load(f)
    assert json.loads(json.dumps(out)) == want
    assert all("words" not in s for o in out for s in o["segments"])


def test_rounds_seek_by_the_last_word_and_clean_up_after_the_word_step(vocab):
    ctx, out = _run(vocab, True)
    plain = _run(vocab, False)[1]
    o = out[0]
    # window 0: single-timestamp ending
    assert o["seeks"][:2] == [0, 3000] == plain[0]["seeks"][:2]
    # window 1: last word end 30 + 6.0 s -> seek 3600 (the timestamp rule alone: 3000 + 1000)
    assert o["seeks"][2] == 3600 and plain[0]["seeks"][2] == 4000
    s1 = [s for s in o["segments"] if s["seek"] == 3000]
    assert len(s1) == 1 and [w["word"] for w in s1[0]["words"]] == [" a", " b"] and s1[0]["words"][-1]["end"] == 36.0
    assert (s1[0]["start"], s1[0]["end"]) == (35.0, 36.0)      # the segment's times follow its first and last word
    # window 2: the last word ends at the window's offset, not behind it: seek by the timestamp, 3600 + 250 * 2
    assert o["seeks"][3] == 4100
    s2 = [s for s in o["segments"] if s["seek"] == 3600]
    assert len(s2) == 1 and s2[0]["start"] == s2[0]["end"] == 36.0 and s2[0]["tokens"] == [] and s2[0]["words"] == []
    # window 3 (seek 4100, 2900 frames left): the clean-up ran on the word-adjusted times
    s3 = [s for s in o["segments"] if s["seek"] == 4100]
    assert len(s3) == 2
    assert s3[0]["tokens"] == [TB + 5, 0, TB + 5] and (s3[0]["start"], s3[0]["end"]) == (41.2, 42.2) and len(s3[0]["words"]) == 1
    assert s3[1]["tokens"] == [] and s3[1]["words"] == [] and s3[1]["start"] == s3[1]["end"] == 42.2 and s3[1]["text"] == ""
    p3 = [s for s in plain[0]["segments"] if s["seek"] == 4500]     # without words the rule clears by the timestamps
    assert p3[0]["tokens"] == [] and p3[1]["tokens"] == [TB + 5, 1, 2, TB + 100]
    # window 3 ends in a single timestamp: the whole window
    assert o["seeks"][4:] == [] and len(o["windows"]) == 4
    # recording 1: its first window is skipped (no segments), the second and last has 2000 frames
    assert [w["skipped"] for w in out[1]["windows"]] == [True, False] and out[1]["seeks"] == [0, 3000]
    assert [w["word"] for w in out[1]["segments"][0]["words"]] == [" a", " b"]
    # recording 2 has ONE content frame: nothing to align to, words [] and the seek of the plain run
    assert out[2]["seeks"] == [0] == plain[2]["seeks"] and [s["words"] for s in out[2]["segments"]] == [[]]
    assert out[2]["segments"][0]["tokens"] == plain[2]["segments"][0]["tokens"] != []
    # one alignment call per round, with the rows of that round's kept windows and each row's own start sequence
    c0 = ctx.align_calls[0]
    assert c0["seek"] == [0] and c0["n_frames"] == [3000] and c0["sot"] == [[SOT, LANG_EN, TASK]] and c0["texts"] == [[0, 1]]
    assert (c0["no_timestamps"], c0["medfilt_width"], c0["qk_scale"], c0["mem"]) == (NO_TS, 7, 1.0, B.WM_MEM_DEVICE)
    c1 = ctx.align_calls[1]
    assert c1["seek"] == [3000, 3000] and c1["n_frames"] == [3000, 2000]
    assert c1["sot"] == [[SOT, LANG_EN, TASK], [SOT, LANG_ZH, TASK]] and c1["texts"] == [[0, 1], [0, 1]]
    assert len(ctx.align_calls) == 4
    # every segment has its id in order and, with a Vocab, its text
    for r in out:
        assert [s["id"] for s in r["segments"]] == list(range(len(r["segments"])))


def test_conditioning_takes_the_tokens_left_after_the_clean_up(vocab):
    ctx, out = _run(vocab, True, condition_on_previous_text=True)
    o = out[0]
    hist = []
    for w in o["windows"]:
        assert w["prompt"] == ([SOT_PREV] + hist[-31:] if hist else []) + [SOT, LANG_EN, TASK]
        hist += [t for s in o["segments"] if s["seek"] == w["seek"] for t in s["tokens"]]
    assert len(o["windows"]) >= 4 and any(not s["tokens"] for s in o["segments"])


def test_word_timestamps_need_a_vocab_and_no_timestamps(vocab):
    recs = [np.zeros(16000, np.float32)]
    with pytest.raises(ValueError):
        B.transcribe_long(FakeCtx({}), recs, word_timestamps=True, no_timestamps=NO_TS, **_fake_kw())
    with pytest.raises(ValueError):
        B.transcribe_long(FakeCtx({}), recs, word_timestamps=True, vocab=vocab, **_fake_kw())


def test_window_segments_without_the_clean_up():
    res = dict(temperature=0.0, avg_logprob=-0.1, compression_ratio=1.0, no_speech_prob=0.0)
    toks = [TB, TB + 3, TB + 3, 10, TB + 6]
    segs, seek, single = B.window_segments(toks, 0, 3000, TB, EOT, res, cleanup=False)
    assert [s["tokens"] for s in segs] == [[TB], [TB + 3], [TB + 3, 10, TB + 6]] and seek == 3000 and single is True
    cleaned, seek2 = B.window_segments(toks, 0, 3000, TB, EOT, res)
    B.clear_empty_segments(segs, EOT)
    assert segs == cleaned and seek2 == seek
    assert B.window_segments([TB, 10, TB + 5, TB + 5, 11], 0, 3000, TB, EOT, res, cleanup=False)[1:] == (10, False)


# ---------------------------------------------------------------- the C ABI without a GPU
def test_align_mel_is_exported_and_rejects_null_arguments(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "wm_align_mel")
    buf = np.zeros(8, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.wm_align_mel(None, p, p, p, p, p, 1, p, 3, 1, 2, p, p, 1, 7, 1.0, p, p, 0) == 1      # WM_ERR_INVALID
    assert b"null" in lib.wm_last_error()
    assert lib.wm_align_mel(None, None, None, None, None, None, 1, None, 3, 1, 2, None, None, 1, 7, 1.0, None, None, 0) == 1
