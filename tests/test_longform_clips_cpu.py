"""CPU tests of transcribe_long's clip_timestamps, hallucination_silence_threshold and carry_initial_prompt on a scripted
fake context, against a restatement of openai-whisper's transcribe() loop for ONE recording written here as that loop is
(a `while` over the clips with `continue`s), plus hand-made cases of every rule.

What the restatement takes from the package: window_segments (the slicing of a window's tokens, tests/test_longform_cpu.py)
and nothing else -- the word step is ref_window_words of tests/test_longform_words_cpu.py, and the clips, the cursor, the
anomaly score, rules H1 - H4, the history and the carried prompt are written out below.

The counter `clip_behind` is this file's reading of "the clip cursor skipping a clip whose start lies behind the seek":
a window's own seek update landed past its clip's end AND past the next clip's start, and the cursor put the seek back to
that start, as openai-whisper's `seek = seek_clips[clip_idx][0]` does."""
import importlib
import math

import numpy as np
import pytest

from test_longform_words_cpu import (BRANCHES as WORD_BRANCHES, EOT, LANG_EN, NO_TS, NS, PIECES, SOT, SOT_PREV, TASK, TB,  # noqa: F401
                                     FakeCtx, ref_window_words, vocab)                                     # (vocab: fixture)

B = importlib.import_module("openai_whisper_coreml_amd.binding")

PUNCT = "\"'“¿([{-\"'.。,，!！?？:：”)]}、"
HOT_T = 0.6          # the first fallback temperature at which a `hot` window is accepted
COUNTERS = ("h1_seek_word", "h1_seek_window", "h2", "before_last", "before_start", "before_window", "after_next",
            "after_anomaly", "after_window", "h3_content", "h3_passed", "h3_fired", "clip_behind", "odd", "dropped_clip",
            "segment_without_words")


def W(tokens, frames, probs=0.5, skip=False, hot=False):
    """One scripted window: generated tokens without eot, start frames of its text tokens + 1 (a longer list is cut), the
    text tokens' probabilities, skipped by the silence rule, accepted only at temperature 0.6."""
    n = len(frames)
    probs = [float(probs)] * n if np.ndim(probs) == 0 else [float(p) for p in probs]
    return dict(tokens=[int(t) for t in tokens], frames=[int(f) for f in frames], probs=probs, skip=skip, hot=hot)


DEFAULT = W([TB, 0, 1, TB + 500], [0, 100, 200])


def _plain(x):
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


class ClipCtx(FakeCtx):
    """FakeCtx with scripted probabilities, fallback (`hot`) and a log of every call with its arguments."""

    def __init__(self, script, n_ctx=64):
        FakeCtx.__init__(self, script, n_ctx)
        self.calls = []
        self.sid_of_base = {}

    def window(self, sid):
        w = self.script.get((int(sid) & 0xFFFF, int(sid) >> 16), None)
        return DEFAULT if w is None else w

    def set_timestamp_rules(self, *a):
        self.calls.append(("set_timestamp_rules", _plain(a)))

    def logmel_long(self, recordings, n_mels=80, device=False):
        self.calls.append(("logmel_long", [len(r) for r in recordings], n_mels, device))
        return FakeCtx.logmel_long(self, recordings, n_mels, device)

    def dev_free(self, p):
        self.calls.append(("dev_free",))

    def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **kw):
        self.calls.append(("transcribe_mel", _plain(mel_base), _plain(mel_len), _plain(seek), _plain(n_frames),
                           [_plain(p) for p in prompts], max_new, sorted((k, _plain(v)) for k, v in kw.items())))
        eot, t = kw["eot"], kw["temperature"]
        ids = kw["sample_ids"]
        n = len(ids)
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.full(n, 0.01, dtype=np.float32)
        for i, sid in enumerate(ids):
            self.sid_of_base[int(mel_base[i])] = int(sid)
            w = self.window(sid)
            body = ([] if w["skip"] else list(w["tokens"])) + [eot]
            assert len(body) <= max_new, (sid, body)
            if w["skip"]:
                ns[i] = 0.9
            toks[i, :len(body)] = body
            lens[i] = len(body)
            lp[i, :len(body)] = -5.0 if w["skip"] or (w["hot"] and t < HOT_T) else -0.1
        return B.TranscribeResult(toks, lens, lp, ns, eot)

    def align_mel(self, mel, mel_base, mel_len, seek, n_frames, text_tokens, sot_seqs, no_timestamps, eot, **kw):
        self.calls.append(("align_mel", _plain(mel_base), _plain(mel_len), _plain(seek), _plain(n_frames),
                           [_plain(t) for t in text_tokens], _plain(sot_seqs), no_timestamps, eot,
                           sorted((k, _plain(v)) for k, v in kw.items())))
        width = max(len(t) for t in text_tokens)
        sf = np.full((len(text_tokens), width + 1), -1, dtype=np.int32)
        pr = np.zeros((len(text_tokens), width), dtype=np.float32)
        for i, (b, t) in enumerate(zip(mel_base, text_tokens)):
            w = self.window(self.sid_of_base[int(b)])
            sf[i, :len(t) + 1] = w["frames"][:len(t) + 1]
            pr[i, :len(t)] = w["probs"][:len(t)]
        return sf, pr


def _kw(**extra):
    kw = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TB, no_speech_token=NS, language=LANG_EN, sot_prev=SOT_PREV,
              compression_ratio_threshold=None)
    kw.update(extra)
    return kw


def _words_kw(vocab, **extra):
    return _kw(vocab=vocab, word_timestamps=True, no_timestamps=NO_TS, **extra)


def _rec(seconds):
    return np.zeros(int(round(16000 * seconds)), np.float32)


def _content(rec):
    return (len(rec) + 480000) // 160 - 3000


# ---------------------------------------------------------------- the restatement: ONE recording, openai-whisper's loop
def ref_word_anomaly_score(word):
    probability = word["probability"]
    duration = word["end"] - word["start"]
    score = 0.0
    if probability < 0.15:
        score += 1.0
    if duration < 0.133:
        score += (0.133 - duration) * 15
    if duration > 2.0:
        score += duration - 2.0
    return score


def ref_is_segment_anomaly(segment):
    if segment is None or not segment["words"]:
        return False
    words = [w for w in segment["words"] if w["word"] not in PUNCT]
    words = words[:8]
    score = sum(ref_word_anomaly_score(w) for w in words)
    return score >= 3 or score + 0.01 >= len(words)


def _next_words_segment(segments):
    return next((s for s in segments if s["words"]), None)


def _get_end(segments):
    return next((w["end"] for s in reversed(segments) for w in reversed(s["words"])), None)


def ref_transcribe(vocab, script, rid, content, times, count, threshold=None, word_timestamps=True, cond=False, ip=(),
                   carry=False, n_ctx=64, h2_keeps_state=True, h4_after_truncation=True):
    """openai-whisper transcribe() for the recording with id `rid`, `content` content frames and clip times `times`
    (seconds) on the scripted windows.  The two flags switch a rule OFF (the hand-made cases show that their scripts can
    tell).  Returns dict(segments, seeks, windows [seek, segment_size, clip, prompt, hallucination?, dropped_segments?])."""
    out = dict(segments=[], seeks=[], windows=[])
    ip = list(ip)
    cap = n_ctx // 2 - 1
    all_tokens = list(ip)
    prompt_reset_since = 0
    last_speech_timestamp = 0.0
    content_duration = content * 0.01
    wcount = dict.fromkeys(WORD_BRANCHES, 0)

    seek_points = [round(t * 100) for t in times]
    if len(seek_points) == 0:
        seek_points.append(0)
    if len(seek_points) % 2 == 1:
        seek_points.append(content)
        count["odd"] += 1
    seek_clips = []
    for k, (a, b) in enumerate(zip(seek_points[::2], seek_points[1::2])):
        a, b = min(a, content), min(b, content)      # project rule: cut to [0, content), drop what is empty
        if a >= b:
            count["dropped_clip"] += 1
            continue
        seek_clips.append((a, b, k))

    clip_idx = 0
    seek = seek_clips[0][0] if seek_clips else 0
    ordinal = 0
    while clip_idx < len(seek_clips):
        seek_clip_start, seek_clip_end, clip_no = seek_clips[clip_idx]
        if seek < seek_clip_start:
            seek = seek_clip_start
        if seek >= seek_clip_end:
            clip_idx += 1
            if clip_idx < len(seek_clips):
                if seek_clips[clip_idx][0] < seek:
                    count["clip_behind"] += 1
                seek = seek_clips[clip_idx][0]
            continue
        time_offset = seek * 0.01
        window_end_time = (seek + 3000) * 0.01
        segment_size = min(3000, content - seek, seek_clip_end - seek)
        segment_duration = segment_size * 0.01

        if cond and carry and ip:
            if len(ip) >= cap:
                text = ip[-cap:]                    # project rule
            else:
                nignored = max(len(ip), prompt_reset_since)
                text = ip + all_tokens[nignored:][-(cap - len(ip)):]
        elif cond:
            text = all_tokens[prompt_reset_since:]
        else:
            text = ip
        prompt = ([SOT_PREV] + text[-cap:] if text else []) + [SOT, LANG_EN, TASK]

        w = script.get((rid, ordinal), None) or DEFAULT
        ordinal += 1
        record = dict(seek=seek, segment_size=segment_size, clip=clip_no, prompt=prompt)
        out["windows"].append(record)
        out["seeks"].append(seek)
        if w["skip"]:
            seek += segment_size
            continue
        temperature = HOT_T if w["hot"] else 0.0
        result = dict(temperature=temperature, avg_logprob=0.0, compression_ratio=0.0, no_speech_prob=0.0)
        previous_seek = seek

        if not word_timestamps:
            current_segments, seek = B.window_segments(w["tokens"], seek, segment_size, TB, EOT, result, vocab)
        else:
            current_segments, seek, single_timestamp_ending = B.window_segments(w["tokens"], seek, segment_size, TB, EOT,
                                                                                result, vocab, cleanup=False)
            text_tokens = [t for s in current_segments for t in s["tokens"] if t < EOT]
            if text_tokens and segment_size >= 2:
                n = len(text_tokens)
                ref_window_words(current_segments, w["frames"][:n + 1], list(np.asarray(w["probs"][:n], np.float32)),
                                 previous_seek, last_speech_timestamp, "en", wcount)
            else:
                for s in current_segments:
                    s["words"] = []
            if not single_timestamp_ending:
                last_word_end = _get_end(current_segments)
                if last_word_end is not None and last_word_end > time_offset:
                    seek = round(last_word_end * 100)

            if threshold is not None:
                if not single_timestamp_ending:                                             # H1
                    last_word_end = _get_end(current_segments)
                    if last_word_end is not None and last_word_end > time_offset:
                        remaining_duration = window_end_time - last_word_end
                        if remaining_duration > threshold:
                            seek = round(last_word_end * 100)
                            count["h1_seek_word"] += 1
                        else:
                            seek = previous_seek + segment_size
                            count["h1_seek_window"] += 1

                first_segment = _next_words_segment(current_segments)                       # H2
                if first_segment is not None and ref_is_segment_anomaly(first_segment):
                    gap = first_segment["start"] - time_offset
                    if gap > threshold:
                        seek = previous_seek + round(gap * 100)
                        count["h2"] += 1
                        record["hallucination"] = "leading"
                        if not h2_keeps_state:
                            last_speech_timestamp = _get_end(current_segments)
                            all_tokens.extend(t for s in current_segments for t in s["tokens"])
                        continue

                hal_last_end = last_speech_timestamp                                        # H3
                for si in range(len(current_segments)):
                    segment = current_segments[si]
                    if not segment["words"]:
                        count["segment_without_words"] += 1
                        continue
                    if ref_is_segment_anomaly(segment):
                        next_segment = _next_words_segment(current_segments[si + 1:])
                        if next_segment is not None:
                            hal_next_start = next_segment["words"][0]["start"]
                        else:
                            hal_next_start = time_offset + segment_duration
                        b1 = segment["start"] - hal_last_end > threshold
                        b2 = segment["start"] < threshold
                        b3 = segment["start"] - time_offset < 2.0
                        a1 = hal_next_start - segment["end"] > threshold
                        a2 = ref_is_segment_anomaly(next_segment)
                        a3 = window_end_time - segment["end"] < 2.0
                        for name, hit in (("before_last", b1), ("before_start", b2), ("before_window", b3),
                                          ("after_next", a1), ("after_anomaly", a2), ("after_window", a3)):
                            count[name] += bool(hit)
                        if (b1 or b2 or b3) and (a1 or a2 or a3):
                            seek = round(max(time_offset + 1, segment["start"]) * 100)
                            if content_duration - segment["end"] < threshold:
                                seek = content
                                count["h3_content"] += 1
                            if not h4_after_truncation:
                                last_speech_timestamp = _get_end(current_segments)
                            record["hallucination"] = "surrounded"
                            record["dropped_segments"] = len(current_segments) - si
                            current_segments[si:] = []
                            count["h3_fired"] += 1
                            break
                        count["h3_passed"] += 1
                    hal_last_end = segment["end"]

            last_word_end = _get_end(current_segments)                                      # H4
            if last_word_end is not None and (h4_after_truncation or record.get("hallucination") != "surrounded"):
                last_speech_timestamp = last_word_end

            for s in current_segments:
                if s["start"] == s["end"] or s["text"].strip() == "":
                    s["text"], s["tokens"], s["words"] = "", [], []

        if cond:
            all_tokens.extend(t for s in current_segments for t in s["tokens"])
            if temperature > 0.5:
                prompt_reset_since = len(all_tokens)
        for s in current_segments:
            s["id"] = len(out["segments"])
            out["segments"].append(s)
    return out


SEGMENT_KEYS = ("id", "seek", "start", "end", "tokens", "text", "temperature")


def _core(out, word_timestamps=True):
    """what the restatement states of a recording's result"""
    keys = SEGMENT_KEYS + (("words",) if word_timestamps else ())
    return dict(segments=[{k: s[k] for k in keys} for s in out["segments"]], seeks=list(out["seeks"]),
                windows=[{k: w[k] for k in ("seek", "segment_size", "clip", "prompt", "hallucination", "dropped_segments")
                          if k in w} for w in out["windows"]])


# ---------------------------------------------------------------- random scripts
_TEXT_P = np.array([4, 4, 4, 1, 1, 1, 1, 1, 0, 0, 0, 4, 2, 1, 1, 1], dtype=np.float64)
_TEXT_P /= _TEXT_P.sum()


def _random_window(rng):
    if rng.random() < 0.06:
        return W([], [0], skip=True)
    n_seg = int(rng.integers(1, 4))
    late = rng.random() < 0.35          # the window's words reach its last seconds
    lead = int(rng.choice([0, 0, 60, 150, 400]))     # frames of silence in front of the first word
    marks = np.sort(rng.integers(1, 1500, size=n_seg + 1))
    toks, frames, probs = [], [], []
    at = lead
    for k in range(n_seg):
        n = int(rng.choice([0, 1, 2, 3, 5], p=[0.1, 0.25, 0.3, 0.25, 0.1]))
        weird = rng.random() < 0.55
        toks += [TB + int(marks[k])] + [int(t) for t in rng.choice(len(PIECES), size=n, p=_TEXT_P)] + [TB + int(marks[k + 1])]
        if k and rng.random() < 0.5:
            at += int(rng.choice([5, 120, 300]))     # a pause between two segments
        for _ in range(n):
            frames.append(at)
            if weird:
                at += int(rng.choice([0, 0, 2, 5, 130]))
                probs.append(float(rng.choice([0.02, 0.1, 0.14, 0.4])))
            else:
                at += int(rng.integers(8, 40))
                probs.append(float(rng.uniform(0.2, 1.0)))
    frames.append(at)
    frames = np.asarray(frames)
    if late and frames[-1] > 0:
        frames = frames + max(0, int(rng.integers(1380, 1500)) - int(frames[-1]))
    frames = np.minimum(frames, 1499)
    ending = rng.choice(["single", "pair", "text"], p=[0.4, 0.3, 0.3])
    if ending == "pair":
        toks.append(toks[-1])
    elif ending == "text":
        toks += [toks[-1], int(rng.integers(0, 3))]
    # (frames and probabilities of text tokens that the slicing drops are never read)
    pad = [int(frames[-1])] * 3
    return W(toks, list(frames) + pad, probs + [0.5] * (len(pad) + 1), hot=rng.random() < 0.08)


class RandomScript:
    """windows made on demand, each from its own seed: the same for everyone who asks"""

    def __init__(self, seed):
        self.seed, self.made = seed, {}

    def get(self, key, default=None):
        if key not in self.made:
            self.made[key] = _random_window(np.random.default_rng([self.seed, key[0], key[1]]))
        return self.made[key]


def _random_times(rng, content):
    n = int(rng.choice([0, 1, 2, 3, 4, 5, 6]))
    t = np.sort(np.round(rng.uniform(0, content / 100 + 4, size=n), 2))
    if n >= 2 and rng.random() < 0.3:
        t[1] = t[0]                     # an empty clip
    if n >= 3 and rng.random() < 0.5:
        t[2] = min(t[2], t[1] + 3.0)    # a clip that starts soon after a short one: overshooting seeks land behind it
    return [float(v) for v in np.sort(t)]


LENGTHS = (70.0, 50.0, 33.21, 0.01, 0.0, 95.5)


def test_random_scripts_match_the_restatement_and_take_every_branch(vocab):
    total = dict.fromkeys(COUNTERS, 0)
    n_windows = n_tags = 0
    recs = [_rec(s) for s in LENGTHS]
    ids = [3, 0, 65535, 9, 12, 1]
    for run in range(40):
        rng = np.random.default_rng(1000 + run)
        script = RandomScript(run)
        times = [_random_times(rng, _content(x)) for x in recs]
        clips = [",".join("%.2f" % t for t in ts) if r % 2 else ts for r, ts in enumerate(times)]
        threshold = [0.5, 2.0, 3.5, None][run % 4]
        cond = run % 3 == 0
        ips = [[1, 2, 0], [], [11] * 40, [2], [0, 1], []] if run % 2 else None
        carry = run % 6 == 3 or run % 6 == 0
        words = threshold is not None or run % 8 == 3
        kw = _words_kw(vocab) if words else _kw(vocab=vocab)
        kw.update(clip_timestamps=clips, hallucination_silence_threshold=threshold, condition_on_previous_text=cond,
                  carry_initial_prompt=carry, recording_ids=ids)
        if ips is not None:
            kw.update(initial_prompt_tokens=ips)
        got = B.transcribe_long(ClipCtx(script), recs, **kw)
        for r, x in enumerate(recs):
            want = ref_transcribe(vocab, script, ids[r], _content(x), times[r], total, threshold, words, cond,
                                  ips[r] if ips is not None else (), carry)
            assert _core(got[r], words) == _core(want, words), (run, r)
            n_windows += len(want["windows"])
            n_tags += sum("hallucination" in w for w in want["windows"])
    print("clips restatement: %d windows, %d tagged, branches %s" % (n_windows, n_tags, total))
    assert all(total[k] > 0 for k in COUNTERS), total


# ---------------------------------------------------------------- hand-made cases: the score and the anomaly
def _word(p, d, text=" a", start=1.0):
    return dict(word=text, start=start, end=start + d, probability=p)


def test_word_score_at_its_three_thresholds():
    assert B.word_anomaly_score(_word(0.15, 1.0)) == 0.0                      # not below 0.15
    assert B.word_anomaly_score(_word(0.1499, 1.0)) == 1.0
    assert B.word_anomaly_score(_word(0.9, 0.133, start=0.0)) == 0.0          # not below 0.133 s
    assert B.word_anomaly_score(_word(0.9, 0.125, start=0.0)) == (0.133 - 0.125) * 15 == 0.12000000000000011
    assert B.word_anomaly_score(_word(0.9, 0.0)) == 0.133 * 15
    assert B.word_anomaly_score(_word(0.9, 2.0)) == 0.0                       # not beyond 2 s
    assert B.word_anomaly_score(_word(0.9, 2.5)) == 0.5
    assert B.word_anomaly_score(_word(0.01, 3.0)) == 2.0                      # the terms add up
    for p, d in ((0.15, 0.133), (0.1, 0.05), (0.5, 7.25)):
        assert B.word_anomaly_score(_word(p, d)) == ref_word_anomaly_score(_word(p, d))


def _seg(words, start=None, end=None):
    return dict(start=words[0]["start"] if start is None else start, end=words[-1]["end"] if end is None else end,
                words=words, tokens=[0] * len(words), text="x")


def test_segment_anomaly_sum_and_count():
    assert B.is_segment_anomaly(None) is False
    assert B.is_segment_anomaly(dict(words=[])) is False
    good, bad = _word(0.9, 0.5), _word(0.1, 0.5)
    assert not B.is_segment_anomaly(_seg([good, good]))
    assert B.is_segment_anomaly(_seg([bad, bad]))                 # 2 + 0.01 >= 2
    assert not B.is_segment_anomaly(_seg([bad, bad, good]))       # 2.01 < 3
    assert B.is_segment_anomaly(_seg([bad, bad, bad, good, good, good]))      # the sum reaches 3
    assert B.is_segment_anomaly(_seg([_word(0.9, 5.0), good, good, good]))    # one word of 5 s: 3
    assert not B.is_segment_anomaly(_seg([_word(0.9, 4.9), good, good, good]))


def test_a_segment_of_punctuation_only_is_anomalous():
    marks = [_word(0.9, 0.5, "."), _word(0.9, 0.5, "?"), _word(0.9, 0.5, "\"'")]     # "\"'": a substring, not a character
    assert B.is_segment_anomaly(_seg(marks))
    assert B.HALLUCINATION_PUNCTUATION == PUNCT == B.PREPEND_PUNCTUATIONS + B.APPEND_PUNCTUATIONS
    assert not B.is_segment_anomaly(_seg(marks + [_word(0.9, 0.5, " a")]))           # the marks do not count: 0.01 < 1
    assert not B.is_segment_anomaly(_seg([_word(0.9, 0.5, " .")]))                   # " ." is no substring


def test_only_the_first_8_words_count():
    good, bad = _word(0.9, 0.5), _word(0.1, 0.5)
    assert not B.is_segment_anomaly(_seg([good] * 8 + [bad] * 20))
    assert B.is_segment_anomaly(_seg([bad] * 8 + [good] * 20))
    assert not B.is_segment_anomaly(_seg([_word(0.9, 0.5, ".")] * 5 + [good] * 8 + [bad] * 20))     # 8 words behind the marks


# ---------------------------------------------------------------- hand-made cases: the rules on one window's segments
def _skip(segments, seek=3000, size=3000, content=20000, thr=2.0, single=True, last=0.0, next_seek=None):
    return B.hallucination_silence_skip(segments, seek, size, content, thr, single, last,
                                        seek + size if next_seek is None else next_seek)


def test_h1_the_last_word_end_or_the_whole_window():
    seg = _seg([_word(0.9, 0.5, start=31.0), _word(0.9, 0.5, start=52.0)])       # last word ends at 52.5; the window at 60
    assert _skip([seg], thr=2.0, single=False, next_seek=4000) == (5250, [seg], None)      # 7.5 s left > 2
    assert _skip([seg], thr=7.5, single=False, next_seek=4000) == (6000, [seg], None)      # not more than 7.5
    assert _skip([seg], thr=8.0, single=False, size=1234, next_seek=4000) == (4234, [seg], None)
    assert _skip([seg], thr=2.0, single=True, next_seek=4000) == (4000, [seg], None)       # a single timestamp ending
    early = _seg([_word(0.9, 0.0, start=30.0)], start=29.0, end=31.0)           # the last word ends AT the window's start
    assert not B.is_segment_anomaly(dict(early, words=[])) and _skip([dict(early, words=[])], single=False, next_seek=3100)[0] == 3100
    assert _skip([early], thr=50.0, single=False, next_seek=3100)[0] == 3100


def test_h2_a_leading_anomaly_discards_the_window():
    bad = _seg([_word(0.1, 0.5, start=34.0), _word(0.1, 0.5, start=34.5)])
    tail = _seg([_word(0.9, 0.5, start=40.0)])
    assert _skip([bad, tail], thr=2.0) == (3400, [], "leading")                  # gap 4 s > 2
    assert _skip([dict(bad, words=[]), bad, tail], thr=3.99)[::2] == (3400, "leading")      # the first segment WITH words
    assert _skip([bad, tail], thr=4.0)[2] != "leading"                           # not more than 4
    good = _seg([_word(0.9, 0.5, start=34.0)])
    assert _skip([good, tail], thr=2.0) == (6000, [good, tail], None)


def test_h3_an_anomaly_between_silences_truncates_the_window():
    good = _seg([_word(0.9, 0.5, start=31.0), _word(0.9, 0.5, start=31.5)])
    bad = _seg([_word(0.1, 0.5, start=40.0), _word(0.1, 0.5, start=40.5)])
    tail = _seg([_word(0.9, 0.5, start=50.0)])
    # silence before (8 s since `good`) and after (9 s to `tail`)
    assert _skip([good, bad, tail], thr=2.0) == (4000, [good], "surrounded")
    # `tail` 1 s behind it and not anomalous, the window's end 19 s away: passed over
    near = _seg([_word(0.9, 0.5, start=42.0)])
    assert _skip([good, bad, near], thr=2.0) == (6000, [good, bad, near], None)
    # ... unless the neighbour is anomalous itself
    near_bad = _seg([_word(0.1, 0.5, start=42.0)])
    assert _skip([good, bad, near_bad], thr=2.0) == (4000, [good], "surrounded")
    # ... or it ends in the window's last 2 s (the window of seek 3000 ends at 60 s)
    late_bad = _seg([_word(0.1, 0.5, start=57.6), _word(0.1, 0.5, start=58.1)])
    assert _skip([good, late_bad], thr=30.0, last=0.0)[2] is None                # no silence before: 26.1 s <= 30
    assert _skip([good, late_bad], thr=20.0) == (5760, [good], "surrounded")
    # no silence before it: it follows `good` directly, starts 2 s into the window or later and not below thr
    close_bad = _seg([_word(0.1, 0.5, start=32.0)])
    assert _skip([good, close_bad], thr=2.0) == (6000, [good, close_bad], None)
    # before: the last speech of the recording counts for the first segment
    assert _skip([close_bad], thr=2.0, last=31.0)[2] is None and _skip([close_bad], thr=2.0, last=29.9)[2] == "surrounded"
    # before: within 2 s of the window's start; the seek moves on by 1 s at least
    edge_bad = _seg([_word(0.1, 0.5, start=30.5)])
    assert _skip([edge_bad], thr=1.0, last=30.0) == (3100, [], "surrounded")
    # before: g.start < thr, a recording that has just begun
    assert _skip([_seg([_word(0.1, 0.5, start=2.5)])], seek=0, thr=3.0, last=2.4) == (250, [], "surrounded")
    # less than thr of the recording behind it: the seek jumps to the end
    assert _skip([good, bad, tail], thr=2.0, content=4290) == (4290, [good], "surrounded")
    assert _skip([good, bad, tail], thr=2.0, content=4300) == (4000, [good], "surrounded")
    # without a later segment with words, the next start is the end of the window's OWN frames
    assert _skip([good, bad], thr=2.0, size=1250)[2] is None                     # 42.5 - 41.0 <= 2
    assert _skip([good, bad], thr=2.0, size=1400)[2] == "surrounded"


def _run(vocab, script, seconds, **extra):
    ctx = ClipCtx(script)
    return ctx, B.transcribe_long(ctx, [_rec(s) for s in seconds], **_words_kw(vocab, **extra))


LEADING = {
    (0, 0): W([TB, 0, 1, TB + 250], [50, 100, 150], 0.9),                        # " a" 1 - 2 s, " b" 2 - 3 s
    (0, 1): W([TB + 500, 0, 1, TB + 600], [500, 500, 500], 0.05),                # two instant words 10 s into the window
    (0, 2): W([TB + 125, 0, 1, TB + 300], [125, 125, 125], 0.05),                # two instant words 2.5 s into the window
}


def test_h2_leaves_the_history_and_the_last_speech_untouched(vocab):
    """Window 1 (seek 3000) is discarded as "leading" and the seek moves by its 10 s gap.  Window 2 (seek 4000) then has an
    anomalous segment at 42.5 s: 2.5 s into the window (H2 needs more than 3, `before_window` less than 2), so with
    threshold 3 it is "surrounded" only by `before_last`: 42.5 - 3.0 (window 0's last word) > 3, where 42.5 - 40.0
    (window 1's) is not."""
    ctx, out = _run(vocab, LEADING, [70.0], hallucination_silence_threshold=3.0, condition_on_previous_text=True)
    o = out[0]
    assert o["seeks"] == [0, 3000, 4000, 4250]
    assert [w.get("hallucination") for w in o["windows"]] == [None, "leading", "surrounded", None]
    assert [w.get("dropped_segments") for w in o["windows"]] == [None, None, 1, None]
    assert [s["seek"] for s in o["segments"]] == [0, 4250] and [s["id"] for s in o["segments"]] == [0, 1]
    first = [TB, 0, 1, TB + 250]
    assert [w["prompt"] for w in o["windows"]][1:3] == [[SOT_PREV] + first + [SOT, LANG_EN, TASK]] * 2
    count = dict.fromkeys(COUNTERS, 0)
    want = ref_transcribe(vocab, LEADING, 0, 7000, [], count, 3.0, cond=True)
    for w in want["windows"]:
        w.pop("clip")
    assert _core(o) == _core(want) and count["h2"] == 1 and count["before_last"] == 1
    off = ref_transcribe(vocab, LEADING, 0, 7000, [], count, 3.0, cond=True, h2_keeps_state=False)
    assert off["seeks"] != o["seeks"] and off["windows"][2]["prompt"] != o["windows"][2]["prompt"]


TRUNCATED = {
    # segment 1: " a" 1 - 2 s, " b" 2 - 3 s (cut at the segment's own end); segment 2: two instant words at 20 s
    (0, 0): W([TB + 50, 0, 1, TB + 150, TB + 1000, 2, 11, TB + 1100], [50, 100, 1000, 1000, 1000], [0.9, 0.9, 0.05, 0.05]),
    (0, 1): W([TB + 125, 0, 1, TB + 300], [125, 125, 125], 0.05),                # two instant words at 22.5 s
}


def test_h4_the_last_speech_follows_the_truncation(vocab):
    """Window 0 drops its second segment (20 s) as "surrounded"; the last speech is then the kept segment's last word
    (3.0 s), not the dropped one's.  Window 1 (seek 2000) shows it as above: 22.5 - 3.0 > 3, 22.5 - 20.0 is not."""
    ctx, out = _run(vocab, TRUNCATED, [70.0], hallucination_silence_threshold=3.0)
    o = out[0]
    assert o["seeks"][:3] == [0, 2000, 2250]
    assert [w.get("hallucination") for w in o["windows"]][:3] == ["surrounded", "surrounded", None]
    assert [(s["seek"], s["start"], s["end"]) for s in o["segments"]][:1] == [(0, 1.0, 3.0)]
    assert o["segments"][0]["words"][-1]["end"] == 3.0 and o["segments"][1]["seek"] == 2250
    count = dict.fromkeys(COUNTERS, 0)
    want = ref_transcribe(vocab, TRUNCATED, 0, 7000, [], count, 3.0)
    for w in want["windows"]:
        w.pop("clip")
    assert _core(o) == _core(want)
    off = ref_transcribe(vocab, TRUNCATED, 0, 7000, [], count, 3.0, h4_after_truncation=False)
    assert off["seeks"][:3] == [0, 2000, 5000] and "hallucination" not in off["windows"][1]


def test_a_threshold_changes_nothing_without_words_to_judge(vocab):
    """windows whose word step does not run (no text token; fewer than 2 frames) keep words [] and today's seek"""
    script = {(0, 0): W([TB, TB + 100, TB + 100, TB + 200], [0]), (1, 0): W([TB, 0, 1], [0, 0, 0], 0.01)}
    ctx, got = _run(vocab, script, [40.0, 0.01], hallucination_silence_threshold=0.0)
    plain = _run(vocab, script, [40.0, 0.01])[1]
    assert got == plain and got[0]["seeks"][:2] == [0, 200] and got[1]["seeks"] == [0]
    assert all("hallucination" not in w for o in got for w in o["windows"])


# ---------------------------------------------------------------- clips
def _calls(vocab, seconds, script=None, words=False, **extra):
    ctx = ClipCtx(script or {})
    kw = _words_kw(vocab, **extra) if words else _kw(vocab=vocab, **extra)
    return ctx.calls, B.transcribe_long(ctx, [_rec(s) for s in seconds], **kw)


def _without_clip(out):
    return [dict(o, windows=[{k: v for k, v in w.items() if k != "clip"} for w in o["windows"]]) for o in out]


def test_defaults_spelled_out_make_the_same_calls(vocab):
    for words in (False, True):
        for cond in (False, True):
            kw = dict(condition_on_previous_text=cond, initial_prompt_tokens=[1, 2])
            calls, out = _calls(vocab, [70.0, 31.5, 0.0], RandomScript(5), words, **kw)
            calls2, out2 = _calls(vocab, [70.0, 31.5, 0.0], RandomScript(5), words, clip_timestamps=None,
                                  hallucination_silence_threshold=None, carry_initial_prompt=False, **kw)
            assert calls == calls2 and out == out2 and len(calls) > 6
            assert all("clip" not in w and "hallucination" not in w for o in out for w in o["windows"])


@pytest.mark.parametrize("words", [False, True])
def test_whole_recording_clips_equal_none(vocab, words):
    seconds = [70.0, 33.33]
    calls, out = _calls(vocab, seconds, RandomScript(7), words)
    assert sum(len(o["windows"]) for o in out) >= 5
    for clip in ("", "0", [], [0], [[0, 70.0], [0, 33.33]], ["0,70", "0, 33.33"], [[], "0"], np.zeros(1), (0.0,)):
        calls2, out2 = _calls(vocab, seconds, RandomScript(7), words, clip_timestamps=clip)
        assert calls2 == calls and _without_clip(out2) == out, clip
        assert all(w["clip"] == 0 for o in out2 for w in o["windows"])


def test_clip_forms_and_windows(vocab):
    """70 s and 50 s; every default window ends in a single timestamp, so a window takes min(3000, what the clip has left)"""
    seconds = [70.0, 50.0]
    flat = _calls(vocab, seconds, clip_timestamps=[5.0, 12.5, 40.0])[1]        # odd: the last clip runs to the end
    assert flat[0]["seeks"] == [500, 4000] and [w["segment_size"] for w in flat[0]["windows"]] == [750, 3000]
    assert flat[1]["seeks"] == [500, 4000] and [w["segment_size"] for w in flat[1]["windows"]] == [750, 1000]
    assert [[w["clip"] for w in o["windows"]] for o in flat] == [[0, 1], [0, 1]]
    assert _calls(vocab, seconds, clip_timestamps="5.0,12.5,40.0")[1] == flat
    assert _calls(vocab, seconds, clip_timestamps=["5,12.5, 40", (5.0, 12.5, 40.0)])[1] == flat
    assert _calls(vocab, seconds, clip_timestamps=np.array([[5.0, 12.5, 40.0]] * 2))[1] == flat
    # one list per recording; a clip is cut at the recording's end, one that is empty after the cut is dropped and keeps
    # its number; a recording without a clip decodes nothing
    calls, per = _calls(vocab, seconds + [20.0], clip_timestamps=[[0, 0, 1.001, 1.004, 65, 200], [60, 70, 80, 90], "20.5"])
    assert per[0]["seeks"] == [6500] and per[0]["windows"][0]["segment_size"] == 500 and per[0]["windows"][0]["clip"] == 2
    assert per[1] == dict(language=LANG_EN, segments=[], seeks=[], windows=[], text="")
    assert per[2]["seeks"] == [] and per[2]["language"] == LANG_EN
    assert [c[0] for c in calls] == ["set_timestamp_rules", "logmel_long", "transcribe_mel", "dev_free"]
    assert calls[2][3:5] == ([6500], [500])
    # the segments of a clipped window lie at the window's offset
    assert flat[0]["segments"][0]["start"] == 5.0 and flat[0]["segments"][0]["seek"] == 500


def test_a_seek_past_the_clip_goes_to_the_next_clip_even_backwards(vocab):
    """a 4 s window whose timestamps say 29 s: the cursor moves to the next clip's start, 6 s"""
    script = {(0, 0): W([TB, 0, TB + 1450, TB + 1450, 1], [0, 10])}
    out = _calls(vocab, [70.0], script, clip_timestamps=[1, 5, 6, 8, 30, 31])[1][0]
    assert out["seeks"] == [100, 600, 3000] and [w["segment_size"] for w in out["windows"]] == [400, 200, 100]
    assert [w["clip"] for w in out["windows"]] == [0, 1, 2]


def test_invalid_clips_are_rejected_before_any_library_call(vocab):
    seconds = [40.0, 35.0]
    bad = [[3.0, 2.0], [-1.0, 2.0], [0.0, float("nan")], [0.0, float("inf")], "5,4", "1,x", [[0, 1]], [[0, 1], [2, 3], [4, 5]],
           [[0, 1], [2, 1]], ["0,1", "-3"]]
    for clip in bad:
        ctx = ClipCtx({})
        with pytest.raises(ValueError):
            B.transcribe_long(ctx, [_rec(s) for s in seconds], clip_timestamps=clip, **_kw(vocab=vocab))
        assert ctx.calls == [], clip
    assert B.clip_times([1, 1, 2.5], 2) == [[1.0, 1.0, 2.5]] * 2                # non-decreasing: equal times are allowed
    assert B.clip_times(5, 2) == B.clip_times(np.float32(5.0), 2) == [[5.0], [5.0]]      # one number is a list of one
    for scalar in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            B.clip_times(scalar, 1)
    assert B.seek_clips([1, 1, 2.5], 1000) == [(250, 1000, 1)] and B.seek_clips([], 0) == []
    assert B.seek_clips([0.014, 0.016, 0.02, 0.5], 10) == [(1, 2, 0), (2, 10, 1)]      # round(t * 100), cut at content


# ---------------------------------------------------------------- carry_initial_prompt
CAP = 31   # n_text_ctx 64


def _prompts(vocab, ip, carry, script=None, **extra):
    out = _calls(vocab, [140.0], script, condition_on_previous_text=True, initial_prompt_tokens=ip,
                 carry_initial_prompt=carry, **extra)[1][0]
    return [w["prompt"] for w in out["windows"]], out


def _history(out, upto):
    """the tokens of the segments of windows 0 .. upto - 1"""
    seeks = out["seeks"][:upto]
    return [t for s in out["segments"] if s["seek"] in seeks for t in s["tokens"]]


@pytest.mark.parametrize("n_ip", [3, CAP - 1, CAP, CAP + 9])
def test_the_carried_prompt_of_every_window(vocab, n_ip):
    ip = [(7 * k) % 16 for k in range(n_ip)]
    got, out = _prompts(vocab, ip, True)
    assert len(got) == 5
    for k, p in enumerate(got):
        hist = _history(out, k)
        assert len(hist) == 4 * k
        if n_ip >= CAP:
            want = ip[-CAP:]
        else:
            want = ip + hist[-(CAP - n_ip):] if hist else ip
        assert p == [SOT_PREV] + want + [SOT, LANG_EN, TASK], (n_ip, k)
        assert len(p) <= 1 + CAP + 3
    off, _ = _prompts(vocab, ip, False)
    if n_ip == 3:      # the history is still short: the initial prompt has not scrolled out yet
        assert got == off
    elif n_ip == CAP - 1:
        assert off[2][1:CAP + 1] == ip[7:] + _history(out, 2) and got[2][1:CAP + 1] == ip + _history(out, 2)[-1:]


def test_the_carried_prompt_after_a_temperature_reset(vocab):
    """window 1 is accepted at temperature 0.6 only: the history restarts behind it, the initial prompt stays"""
    script = {(0, 1): W([TB, 2, 11, TB + 500], [0, 100, 200], hot=True)}
    ip = [5, 6, 7]
    got, out = _prompts(vocab, ip, True, script)
    assert [w["temperatures"] for w in out["windows"]][:3] == [[0.0], [0.0, 0.2, 0.4, 0.6], [0.0]]
    d = [TB, 0, 1, TB + 500]
    tail = [SOT, LANG_EN, TASK]
    assert got[0] == [SOT_PREV] + ip + tail
    assert got[1] == [SOT_PREV] + ip + d + tail
    assert got[2] == [SOT_PREV] + ip + tail                      # prompt_reset_since = 3 + 8 > len(ip)
    assert got[3] == [SOT_PREV] + ip + d + tail
    off, _ = _prompts(vocab, ip, False, script)
    assert off[2] == tail and off[3] == [SOT_PREV] + d + tail   # without the flag the prompt is gone after the reset


def test_carry_off_or_without_meaning_is_todays_prompt(vocab):
    for kw in (dict(initial_prompt_tokens=[1, 2, 3]), dict(condition_on_previous_text=True),
               dict(condition_on_previous_text=True, initial_prompt_tokens=[[], []]),
               dict(initial_prompt_tokens=[[4], [5, 6]])):
        calls, out = _calls(vocab, [70.0, 40.0], RandomScript(3), **kw)
        calls2, out2 = _calls(vocab, [70.0, 40.0], RandomScript(3), carry_initial_prompt=True, **kw)
        assert calls == calls2 and out == out2, kw
    # per recording: only the one with a prompt carries it
    out = _calls(vocab, [100.0, 100.0], condition_on_previous_text=True, carry_initial_prompt=True,
                 initial_prompt_tokens=[[9] * 29, []])[1]
    assert all(w["prompt"][:30] == [SOT_PREV] + [9] * 29 for w in out[0]["windows"])
    assert out[1]["windows"][0]["prompt"] == [SOT, LANG_EN, TASK] and out[1]["windows"][3]["prompt"][0] == SOT_PREV
    assert 9 not in out[1]["windows"][3]["prompt"]
    with pytest.raises(ValueError):
        B.transcribe_long(ClipCtx({}), [_rec(40.0)], condition_on_previous_text=True, carry_initial_prompt=True,
                          initial_prompt_tokens=[1], **_kw(vocab=vocab, sot_prev=None))


def test_carried_prompt_leaves_conditioned_prompt_alone():
    seq = [SOT, LANG_EN, TASK]
    hist = list(range(100, 160))
    assert B.conditioned_prompt(hist, 0, seq, SOT_PREV, 64) == [SOT_PREV] + hist[-31:] + seq
    assert B.conditioned_prompt(hist, 60, seq, SOT_PREV, 64) == seq
    assert B.carried_prompt(hist[:4], hist, 0, seq, SOT_PREV, 64) == [SOT_PREV] + hist[:4] + hist[-27:] + seq
    assert B.carried_prompt(hist[:4], hist, 58, seq, SOT_PREV, 64) == [SOT_PREV] + hist[:4] + hist[58:] + seq
    assert B.carried_prompt(hist[:4], hist, 60, seq, SOT_PREV, 64) == [SOT_PREV] + hist[:4] + seq
    assert B.carried_prompt(hist[:4], hist, 2, seq, SOT_PREV, 64) == B.carried_prompt(hist[:4], hist, 4, seq, SOT_PREV, 64)
    assert B.carried_prompt(hist[:30], hist, 0, seq, SOT_PREV, 64) == [SOT_PREV] + hist[:30] + hist[-1:] + seq
    assert B.carried_prompt(hist[:31], hist, 0, seq, SOT_PREV, 64) == [SOT_PREV] + hist[:31] + seq
    assert B.carried_prompt(hist[:40], hist, 0, seq, SOT_PREV, 64) == [SOT_PREV] + hist[9:40] + seq


# ---------------------------------------------------------------- errors
def test_threshold_errors(vocab):
    recs = [_rec(40.0)]
    for kw in (_kw(vocab=vocab, hallucination_silence_threshold=2.0),            # without word_timestamps
               _words_kw(vocab, hallucination_silence_threshold=-0.5),
               _words_kw(vocab, hallucination_silence_threshold=float("inf")),
               _words_kw(vocab, hallucination_silence_threshold=float("nan"))):
        ctx = ClipCtx({})
        with pytest.raises(ValueError):
            B.transcribe_long(ctx, recs, **kw)
        assert ctx.calls == []
    assert math.isfinite(0.0) and B.transcribe_long(ClipCtx({}), recs, **_words_kw(vocab, hallucination_silence_threshold=0))


def test_a_seek_that_does_not_grow_is_an_error_not_a_hang(vocab):
    """<|0.00|><|0.00|> at the end of a window is a seek update of zero frames"""
    with pytest.raises(AssertionError):
        B.transcribe_long(ClipCtx({(0, 1): W([TB, 0, TB, TB], [0, 0])}), [_rec(70.0)], clip_timestamps=None, **_kw(vocab=vocab))
