"""Characterization of binding.transcribe_long on a recording fake context: for every mode of the function, the complete
log of the Context calls it makes -- (name, positional values, sorted keyword items) -- and the dicts it returns, compared
with tests/golden/longform_calls_parent.json.

The golden is this project's own recorded result: `python tests/test_longform_calls_cpu.py --record <commit>` run at the
commit BEFORE transcribe_long was restructured into units / row sources (the commit is named inside the file).  It is not to
be recorded again from later code: a difference is a change of behaviour.  The smallest case of every group keeps its whole
log in the file; the others keep the sha256 of the canonical JSON.

Every case holds a window that needs a fallback step and a skipped window (asserted by the recorder)."""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from test_align_cpu import _bytes_to_unicode
from test_longform_clips_cpu import DEFAULT, HOT_T, LEADING, W, _plain, _rec
from test_longform_words_cpu import EOT, LANG_EN, LANG_ZH, NO_TS, NS, PIECES, SOT, SOT_PREV, TASK, TB

B = importlib.import_module("openai_whisper_coreml_amd.binding")
GOLDEN_FILE = os.path.join(GOLDEN, "longform_calls_parent.json")


def canon(x):
    """_plain, plus the things a call log meets: pointers, sets, big arrays (shape and dtype), dicts, NaN"""
    if isinstance(x, ctypes.c_void_p):
        return "ptr:%d" % (x.value or 0)
    if isinstance(x, FakeSet):
        return "set:%d" % x.number
    if isinstance(x, np.ndarray) and x.size > 64:
        return dict(shape=list(x.shape), dtype=str(x.dtype))
    if isinstance(x, dict):
        return {str(k): canon(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, type):
        return str(np.dtype(x))
    x = _plain(x)
    if isinstance(x, float) and x != x:
        return "nan"
    return x


class FakeSet:
    def __init__(self, ctx, number):
        self.ctx, self.number, self.sid = ctx, number, {}

    def close(self):
        self.ctx.calls.append(["set.close", [canon(self)], []])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RecCtx:
    """Every method takes *a, **kw and logs them.  script[(recording id, sample id >> 16)] = W(...): the decode and the
    alignment of the row with that sample id; DEFAULT without an entry.  fail_at: the decode call that raises."""

    def __init__(self, script, n_ctx=64, tracks=None, fail_at=None):
        self.dims = dict(n_text_ctx=n_ctx, n_mels=80, n_vocab=1 << 16)   # (timestamp ids need 2 bytes)
        self.script, self.tracks, self.fail_at = script, tracks, fail_at
        self.calls, self.sid_of, self.n_sets, self.n_decodes = [], {}, 0, 0

    def _log(self, name, a, kw):
        self.calls.append([name, canon(a), sorted([k, canon(v)] for k, v in kw.items())])

    def window(self, sid):
        return self.script.get((int(sid) & 0xFFFF, int(sid) >> 16)) or DEFAULT

    @staticmethod
    def _mel_layout(lengths, n_mels):
        T = np.array([(int(n) + 480000) // 160 for n in lengths], dtype=np.int32)
        return np.concatenate([[0], np.cumsum(T.astype(np.int64) * n_mels)]).astype(np.int64), T

    def set_timestamp_rules(self, *a, **kw):
        self._log("set_timestamp_rules", a, kw)

    def logmel_long(self, *a, **kw):
        self._log("logmel_long", a, kw)
        offs, T = self._mel_layout([len(r) for r in a[0]], kw["n_mels"])
        return ctypes.c_void_p(4096), offs, T

    def resample_16k(self, *a, **kw):
        self._log("resample_16k", a, kw)
        n = [-(-len(r) * 16000 // int(sr)) for r, sr in zip(a[0], a[1])]
        return ctypes.c_void_p(8192), np.concatenate([[0], np.cumsum(n)]).astype(np.int64)

    def logmel_long_device(self, *a, **kw):
        self._log("logmel_long_device", a, kw)
        offs, T = self._mel_layout(np.diff(a[2]), kw["n_mels"])
        return ctypes.c_void_p(4096), offs, T

    def vad_energy(self, *a, **kw):
        self._log("vad_energy", a, kw)
        assert [len(t) for t in self.tracks] == [int(n) for n in a[3]]
        return [np.asarray(t, dtype=np.float32) for t in self.tracks]

    def dev_free(self, *a, **kw):
        self._log("dev_free", a, kw)

    def _decode(self, ids, max_new, kw):
        self.n_decodes += 1
        if self.fail_at == self.n_decodes:
            raise RuntimeError("scripted failure of decode call %d" % self.n_decodes)
        eot, t = kw["eot"], kw["temperature"]
        n = len(ids)
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.full(n, 0.01, dtype=np.float32)
        for i, sid in enumerate(ids):
            w = self.window(sid)
            body = ([] if w["skip"] else list(w["tokens"])) + [eot]
            assert len(body) <= max_new, (sid, body)
            if w["skip"]:
                ns[i] = 0.9
            toks[i, :len(body)] = body
            lens[i] = len(body)
            lp[i, :len(body)] = -5.0 if w["skip"] or (w["hot"] and t < HOT_T) else -0.1
        r = B.TranscribeResult(toks, lens, lp, ns, eot)
        if "best_of" in kw:
            r.candidate = np.array([(int(s) >> 16) % kw["best_of"] for s in ids], dtype=np.int32)
        if "beam_size" in kw:
            r.hypothesis = np.array([(int(s) + 1) % kw["beam_size"] for s in ids], dtype=np.int32)
        return r

    def transcribe_mel(self, *a, **kw):
        self._log("transcribe_mel", a, kw)
        for b, s, sid in zip(a[1], a[3], kw["sample_ids"]):
            self.sid_of[(int(b), int(s))] = int(sid)
        return self._decode(kw["sample_ids"], a[6], kw)

    def encode_windows(self, *a, **kw):
        self._log("encode_windows", a, kw)
        self.n_sets += 1
        return FakeSet(self, self.n_sets)

    def transcribe_windows(self, *a, **kw):
        self._log("transcribe_windows", a, kw)
        for row, sid in zip(a[1], kw["sample_ids"]):
            a[0].sid[int(row)] = int(sid)
        return self._decode(kw["sample_ids"], a[3], kw)

    def _align(self, sids, text_tokens):
        width = max(len(t) for t in text_tokens)
        sf = np.full((len(text_tokens), width + 1), -1, dtype=np.int32)
        pr = np.zeros((len(text_tokens), width), dtype=np.float32)
        for i, (sid, t) in enumerate(zip(sids, text_tokens)):
            w = self.window(sid)
            sf[i, :len(t) + 1] = w["frames"][:len(t) + 1]
            pr[i, :len(t)] = w["probs"][:len(t)]
        return sf, pr

    def align_mel(self, *a, **kw):
        self._log("align_mel", a, kw)
        return self._align([self.sid_of[(int(b), int(s))] for b, s in zip(a[1], a[3])], a[5])

    def align_windows(self, *a, **kw):
        self._log("align_windows", a, kw)
        return self._align([a[0].sid[int(r)] for r in a[1]], a[2])

    def windows_detect_language(self, *a, **kw):
        self._log("windows_detect_language", a, kw)
        rows = np.asarray(a[1])
        return (rows % 2).astype(np.int32), None


def make_vocab(directory):
    b2u = _bytes_to_unicode()
    path = os.path.join(str(directory), "vocab.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"".join(b2u[c] for c in p.encode()): i for i, p in enumerate(PIECES)}, f)
    return B.Vocab(path)


# ---------------------------------------------------------------- the cases
SECONDS = (70.0, 37.5, 0.01)        # 7000, 3750 and 1 content frames: the last is shorter than a window (and than 2 frames)
CONTENT = (7000, 3750, 1)
HOT = W(DEFAULT["tokens"], DEFAULT["frames"], hot=True)
SKIP = W([], [0], skip=True)
NO_TEXT = W([TB, TB + 100, TB + 100, TB + 200], [0])     # timestamps only: kept, nothing to align
PAST = W([TB, 0, TB + 600, TB + 600, 1], [0, 10, 20])          # no single ending: its timestamps put the seek 1200 frames on
# keys are (recording id, window ordinal) -- and, with parallel_clips, (recording id, clip << 4 | window within the clip)
SCRIPT = {(0, 1): HOT, (0, 2): NO_TEXT, (1, 0): SKIP, (1, 16): SKIP, (0, 16): HOT, (0, 32): HOT}
CLIP_SCRIPT = {**SCRIPT, (0, 0): PAST}
HAL_SCRIPT = {**LEADING, (1, 0): SKIP, (1, 1): HOT}
MIN = dict(sot=SOT, task=TASK, eot=EOT, timestamp_begin=TB, no_speech_token=NS, language=LANG_EN)
STD = dict(MIN, sot_prev=SOT_PREV, compression_ratio_threshold=None)
LANGS = [LANG_EN, LANG_ZH, LANG_EN]
LONG_PROMPT = [i % 16 for i in range(33)]                      # more than n_ctx // 2 - 1 = 31 tokens
PER_REC_CLIPS = [[0.0, 4.0, 20.0, 75.0, 80.0, 85.0], "0,3", []]   # (cut at the content; dropped by the cut), string, none


def _tracks():
    y0 = np.zeros(CONTENT[0], np.float32)
    for a, b in ((300, 900), (1500, 1600), (4000, 6900)):
        y0[a:b] = 5.0
    return [y0, np.full(CONTENT[1], 1.0, np.float32), np.zeros(CONTENT[2], np.float32)]


def _stereo(seconds, rate):
    return np.zeros((int(round(rate * seconds)), 2), np.int16)


def cases(vocab):
    """name -> dict(kw, script, [ctx: RecCtx keywords], [recs], [full: keep the whole log in the golden])"""
    words = dict(STD, vocab=vocab, word_timestamps=True, no_timestamps=NO_TS, language=LANGS)
    c = {}

    def add(name, kw, script=SCRIPT, full=False, **more):
        c[name] = dict(kw=kw, script=script, full=full, **more)

    add("defaults", MIN, full=True)
    add("flat_prompt", dict(STD, initial_prompt_tokens=[3, 4, 5]), full=True)
    add("per_recording_prompts", dict(STD, initial_prompt_tokens=[[3, 4], [], [5]]), full=True)
    add("cond", dict(STD, condition_on_previous_text=True), full=True)
    add("cond_prompts", dict(STD, condition_on_previous_text=True, initial_prompt_tokens=[[3, 4], [], LONG_PROMPT]))
    add("cond_carry", dict(STD, condition_on_previous_text=True, carry_initial_prompt=True,
                           initial_prompt_tokens=[[3, 4], [], LONG_PROMPT]))
    add("cond_carry_flat_long", dict(STD, condition_on_previous_text=True, carry_initial_prompt=True,
                                     initial_prompt_tokens=LONG_PROMPT, prompt_reset_on_temperature=0.7))
    add("cond_vocab", dict(STD, condition_on_previous_text=True, vocab=vocab, compression_ratio_threshold="auto"))
    add("words", words, full=True)
    add("words_punctuations", dict(words, prepend_punctuations="(", append_punctuations=".,"))
    add("words_cond_hallucination", dict(words, language=LANG_EN, condition_on_previous_text=True,
                                         hallucination_silence_threshold=3.0), script=HAL_SCRIPT, full=True)
    add("words_hallucination_zero", dict(words, hallucination_silence_threshold=0.0), script=HAL_SCRIPT)
    add("best_of", dict(STD, best_of=3, length_penalty=0.5), full=True)
    add("best_of_ragged", dict(STD, best_of=2, condition_on_previous_text=True))
    add("beam", dict(STD, beam_size=2, patience=1.5), full=True)
    add("beam_best_of_cond", dict(STD, beam_size=3, best_of=2, length_penalty=1.0, condition_on_previous_text=True))
    add("reuse", dict(STD, reuse_encoder=True), full=True)
    add("reuse_words", dict(words, reuse_encoder=True))
    add("reuse_words_cond", dict(words, reuse_encoder=True, condition_on_previous_text=True))
    add("reuse_best_of", dict(STD, reuse_encoder=True, best_of=3))
    add("reuse_beam", dict(STD, reuse_encoder=True, beam_size=2, patience=2.0, length_penalty=0.3))
    add("reuse_detect_language", dict(STD, reuse_encoder=True, language=None, lang_first=LANG_EN, lang_last=LANG_EN + 3),
        full=True)
    add("clips_string", dict(STD, clip_timestamps="1,5,10,12"), script=CLIP_SCRIPT, full=True)
    add("clips_flat_odd", dict(STD, clip_timestamps=[1.0, 5.0, 33.0]), script=CLIP_SCRIPT)
    add("clips_per_recording", dict(STD, clip_timestamps=PER_REC_CLIPS), script=CLIP_SCRIPT)
    add("clips_words", dict(words, clip_timestamps=PER_REC_CLIPS, hallucination_silence_threshold=2.0), script=CLIP_SCRIPT)
    add("vad_true", dict(STD, vad=True), ctx=dict(tracks=_tracks()), full=True)
    add("vad_overrides", dict(STD, vad=dict(band=(0, 80), smooth=11, params=dict(speech_pad=0, min_speech=3), max_frames=100)),
        ctx=dict(tracks=_tracks()))
    add("vad_false", dict(STD, vad=False))
    add("parallel_2_clips", dict(STD, parallel_clips=2, clip_timestamps=PER_REC_CLIPS), script=CLIP_SCRIPT, full=True)
    add("parallel_true_clips", dict(STD, parallel_clips=True, clip_timestamps="1,5,10,12,30,69"), script=CLIP_SCRIPT)
    add("parallel_true_vad", dict(STD, parallel_clips=True, vad=True), ctx=dict(tracks=_tracks()))
    add("parallel_2_vad_words_reuse", dict(words, parallel_clips=2, vad=True, reuse_encoder=True), ctx=dict(tracks=_tracks()))
    add("parallel_3_words_ids", dict(words, parallel_clips=3, clip_timestamps=PER_REC_CLIPS, recording_ids=[7, 300, 65535]),
        script={**CLIP_SCRIPT, (7, 0): PAST, (7, 16): HOT, (300, 0): SKIP})
    add("parallel_1_reuse_best_of", dict(STD, parallel_clips=1, reuse_encoder=True, best_of=2, beam_size=2))
    add("sample_rates", dict(STD, sample_rates=[8000, 44100, 16000]), full=True,
        recs=[_stereo(70.0, 8000), np.zeros(int(44100 * 37.5), np.float32), np.zeros(160, np.int16)])
    add("sample_rates_reuse_words", dict(words, sample_rates=[16000, 16000, 16000], reuse_encoder=True))
    add("no_recordings", STD, recs=[], full=True)
    add("no_recordings_sample_rates", dict(STD, sample_rates=[1]), recs=[], full=True)
    add("decode_raises_in_a_reuse_round", dict(words, reuse_encoder=True), ctx=dict(fail_at=3), full=True)
    add("decode_raises_in_the_first_round", dict(STD, reuse_encoder=True, sample_rates=[16000] * 3), ctx=dict(fail_at=1))
    add("decode_raises_without_reuse", STD, ctx=dict(fail_at=2))
    # every ValueError of the function, in the order of its checks
    for name, kw in (
            ("patience_without_beam", dict(STD, patience=2.0)),
            ("beam_size_range", dict(STD, beam_size=9)),
            ("beam_candidates_range", dict(STD, beam_size=8, patience=3.0)),
            ("recording_ids_count", dict(STD, recording_ids=[0, 1])),
            ("recording_ids_range", dict(STD, recording_ids=[0, 1, 65536])),
            ("cond_without_sot_prev", dict(MIN, condition_on_previous_text=True)),
            ("per_recording_prompts_count", dict(STD, initial_prompt_tokens=[[1], [2]])),
            ("words_without_vocab", dict(STD, word_timestamps=True, no_timestamps=NO_TS)),
            ("words_without_no_timestamps", dict(STD, word_timestamps=True, vocab=vocab)),
            ("clips_decreasing", dict(STD, clip_timestamps=[5.0, 1.0])),
            ("clips_not_finite", dict(STD, clip_timestamps="1,inf")),
            ("clips_count", dict(STD, clip_timestamps=[[0.0], [1.0]])),
            ("vad_with_clips", dict(STD, vad=True, clip_timestamps="")),
            ("vad_override_name", dict(STD, vad=dict(bands=(0, 1)))),
            ("parallel_false", dict(STD, parallel_clips=False)),
            ("parallel_zero", dict(STD, parallel_clips=0)),
            ("parallel_with_cond", dict(STD, parallel_clips=2, condition_on_previous_text=True)),
            ("parallel_with_hallucination", dict(words, parallel_clips=2, hallucination_silence_threshold=2.0)),
            ("hallucination_not_finite", dict(words, hallucination_silence_threshold=float("inf"))),
            ("hallucination_negative", dict(words, hallucination_silence_threshold=-1.0)),
            ("hallucination_without_words", dict(STD, hallucination_silence_threshold=1.0)),
            ("sample_rates_count", dict(STD, sample_rates=[16000])),
            ("detect_without_lang_range", dict(STD, language=None)),
            ("detect_without_lang_range_reuse", dict(STD, language=None, lang_first=LANG_EN, reuse_encoder=True,
                                                     sample_rates=[16000] * 3)),
            ("language_count", dict(STD, language=[LANG_EN])),
            ("prompt_without_sot_prev", dict(MIN, initial_prompt_tokens=[1, 2])),
            ("per_recording_prompts_without_sot_prev", dict(MIN, initial_prompt_tokens=[[1], [], [2]])),
            ("compression_ratio_threshold_name", dict(STD, compression_ratio_threshold="automatic")),
            ("compression_ratio_threshold_name_reuse", dict(STD, compression_ratio_threshold="automatic", reuse_encoder=True))):
        add("error_" + name, kw, full=True)
    add("error_vad_param_name", dict(STD, vad=dict(params=dict(nothing=1))), ctx=dict(tracks=_tracks()), full=True)
    return c


def run_case(case):
    """dict(calls, out) or dict(calls, error) of one case, as JSON would hand it back"""
    ctx = RecCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    got = dict(calls=ctx.calls)
    try:
        got["out"] = B.transcribe_long(ctx, recs, **case["kw"])
    except (ValueError, RuntimeError) as e:
        got["error"] = [type(e).__name__, str(e)]
    return json.loads(json.dumps(canon(got)))


def digest(got):
    return hashlib.sha256(json.dumps(got, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def _vocab_case_names():
    return sorted(cases(None))


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_golden_holds_every_case(golden):
    assert sorted(golden["cases"]) == _vocab_case_names()


@pytest.mark.parametrize("name", _vocab_case_names())
def test_calls_and_results_are_the_parents(vocab, golden, name):
    case = cases(vocab)[name]
    got = run_case(case)
    want = golden["cases"][name]
    assert ("error" in got) == name.startswith(("error_", "decode_raises"))
    if "full" in want:
        assert got["calls"] == want["full"]["calls"]
        assert got == want["full"]
    assert digest(got) == want["sha256"]


def test_a_failed_decode_closes_the_set_and_frees_the_mel(vocab):
    got = run_case(cases(vocab)["decode_raises_in_a_reuse_round"])
    assert got["error"][0] == "RuntimeError"
    assert [c[0] for c in got["calls"][-2:]] == ["set.close", "dev_free"]
    assert sum(c[0] == "encode_windows" for c in got["calls"]) == sum(c[0] == "set.close" for c in got["calls"])


def test_the_detected_language_path_without_reuse_goes_through_the_context(vocab):
    """language=None without reuse_encoder: n_mels x R downloads of 4 x 3000 bytes (row c of recording r's mel, frames
    [0, 3000)), then encode_mel, then detect_language_probs -- all of them Context methods, so a fake reaches the path."""
    class LidCtx(RecCtx):
        lib = handle = None   # (not to be touched)

        def download(self, *a, **kw):
            self._log("download", a, kw)
            return np.zeros(a[1], dtype=a[2])

        def encode_mel(self, *a, **kw):
            self._log("encode_mel", a, kw)
            return np.zeros((len(a[0]), 2, 2), np.float32)

        def detect_language_probs(self, *a, **kw):
            self._log("detect_language_probs", canon(a[1:]), kw)
            return np.arange(len(a[0]), dtype=np.int32) % 2, None

    ctx = LidCtx(SCRIPT)
    out = B.transcribe_long(ctx, [_rec(s) for s in SECONDS], **dict(STD, language=None, lang_first=LANG_EN, lang_last=LANG_ZH))
    assert [o["language"] for o in out] == [LANG_EN, LANG_ZH, LANG_EN]
    names = [c[0] for c in ctx.calls]
    assert names[:2] == ["set_timestamp_rules", "logmel_long"] and names[2:242] == ["download"] * 240
    offs, T = RecCtx._mel_layout([len(_rec(s)) for s in SECONDS], 80)
    want = ["ptr:%d" % (4096 + 4 * (int(offs[r]) + c * int(T[r]))) for r in range(3) for c in range(80)]
    assert [c[1][0] for c in ctx.calls[2:242]] == want
    assert all(int(np.prod(c[1][1])) * np.dtype(c[1][2]).itemsize == 4 * 3000 and c[2] == [] for c in ctx.calls[2:242])
    assert ctx.calls[242] == ["encode_mel", [dict(shape=[3, 80, 3000], dtype="float32")], []]
    assert ctx.calls[243] == ["detect_language_probs", [SOT, LANG_EN, LANG_ZH], []]
    assert names[244] == "transcribe_mel" and names[-1] == "dev_free"
    # behind the language step the run is the one with these languages given
    given = run_case(dict(kw=dict(STD, language=LANGS), script=SCRIPT))
    assert json.loads(json.dumps(canon(ctx.calls[244:]))) == given["calls"][2:]
    assert json.loads(json.dumps(canon(out))) == given["out"]


def record(commit):
    """Write the golden from the code as it stands: for the parent commit only (see the module's docstring)."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        vocab = make_vocab(d)
        out = dict(recorded_at=commit, cases={})
        for name, case in sorted(cases(vocab).items()):
            got = run_case(case)
            assert ("error" in got) == name.startswith(("error_", "decode_raises")), (name, got.get("error"))
            if "out" in got and got["out"]:
                windows = [w for o in got["out"] for w in o["windows"]]
                assert any(len(w["temperatures"]) > 1 for w in windows), name
                assert any(w["skipped"] for w in windows), name
            out["cases"][name] = dict(sha256=digest(got))
            if case["full"]:
                out["cases"][name]["full"] = got
        vocab.close()
    with open(GOLDEN_FILE, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d bytes" % (GOLDEN_FILE, len(out["cases"]), os.path.getsize(GOLDEN_FILE)))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        raise SystemExit("usage: python tests/test_longform_calls_cpu.py --record <commit the golden is recorded at>")
    record(sys.argv[2])
