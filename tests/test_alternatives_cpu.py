"""Top-n alternatives and entropy (wm_request_alternatives) without a device: the numpy restatement
(tests/alt_ref.py) on hand-worked rows and against the beam tests' own restatement, the seeded rows' sum-rule gaps that
tests/test_alternatives_kernel_gpu.py relies on, the wrappers' packing and ValueErrors against a stand-in library, and
transcribe_long's calls on the recording fake of test_longform_calls_cpu.py."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import alt_ref as A
from test_beam_kernel_gpu import _lists_np
from test_binding_calls_cpu import BASE3, FakeLib, LEN3, MEL, NF3, P3, RAGGED, SEEK3, SET_HANDLE, _at
from test_longform_calls_cpu import RecCtx, SECONDS, canon, cases, make_vocab, run_case
from test_longform_clips_cpu import _rec

B = importlib.import_module("openai_whisper_coreml_amd.binding")
LN2 = math.log(2.0)


# ---------------------------------------------------------------- the restatement on hand-worked rows
def row_of(probs, shift=2.0):
    """logits whose softmax over the listed ids is `probs` exactly (0: -inf)"""
    with np.errstate(divide="ignore"):
        return (np.log(np.asarray(probs, np.float64)) + shift).astype(np.float64)


def test_order_logprobs_counts_and_entropy_by_hand():
    v = row_of([0.125, 0.5, 0.25, 0.125])
    r = A.alternatives_np(v, 3)
    assert r.ids.tolist() == [1, 2, 0] and r.count == 3 and r.size == 4       # the tie at 0.125: the lower id
    assert np.allclose(r.logprobs, [-LN2, -2 * LN2, -3 * LN2], rtol=0, atol=1e-12)
    assert abs(r.entropy - 1.75 * LN2) < 1e-12                                 # 0.5 * 1 + 0.25 * 2 + 2 * 0.125 * 3 bits
    assert A.alternatives_np(v, 16).ids.tolist() == [1, 2, 0, 3] and A.alternatives_np(v, 16).count == 4   # fewer than n
    assert A.alternatives_np(v, 1).ids.tolist() == [1]
    # exact ties at the top: ascending ids
    t = np.array([1.0, 3.0, 3.0, 0.0, 3.0])
    assert A.alternatives_np(t, 4).ids.tolist() == [1, 2, 4, 0]
    assert len(set(A.alternatives_np(t, 3).logprobs.tolist())) == 1


def test_minus_infinity_suppressed_ids_and_the_empty_set():
    v = row_of([0.5, 0.0, 0.25, 0.25])
    r = A.alternatives_np(v, 4)
    assert r.ids.tolist() == [0, 2, 3] and r.count == 3 and abs(r.entropy - 1.5 * LN2) < 1e-12      # -inf is never listed
    big = v.copy()
    big[1] = 1e6                                                                                   # a suppressed id, however large
    r2 = A.alternatives_np(big, 4, suppress=[1])
    assert r2.ids.tolist() == [0, 2, 3] and np.allclose(r2.logprobs, r.logprobs) and abs(r2.entropy - r.entropy) < 1e-12
    one = A.alternatives_np(v, 4, suppress=[0, 2])
    assert one.ids.tolist() == [3] and one.logprobs.tolist() == [0.0] and one.entropy == 0.0
    none = A.alternatives_np(np.full(8, -np.inf), 4)
    assert none.count == 0 and none.ids.size == 0 and none.entropy == 0.0 and none.size == 0
    assert A.alternatives_np(v, 4, suppress=[0, 2, 3]).count == 0
    tok, lp, cnt, ent = A.packed([r, none, one], 4)
    assert tok.tolist() == [[0, 2, 3, -1], [-1] * 4, [3, -1, -1, -1]] and cnt.tolist() == [3, 0, 1]
    assert lp[1].tolist() == [0.0] * 4 and ent[1] == 0.0 and lp[0, 3] == 0.0


def test_the_sum_rule_by_hand():
    """ids 0 .. 3 text, 4 .. 7 timestamps.  Text best 0.3; the timestamps hold 0.4 together: a timestamp is forced and the list
    holds timestamps only, renormalised.  With 0.25 together they are not, and the list is over everything allowed."""
    forced = row_of([0.3, 0.2, 0.1, 0.0, 0.1, 0.1, 0.1, 0.1])
    r = A.alternatives_np(forced, 3, rng=(0, 4, 4, 8))
    assert r.gap > 0 and abs(r.gap - math.log(0.4 / 0.3)) < 1e-12
    assert r.ids.tolist() == [4, 5, 6] and r.size == 4 and np.allclose(r.logprobs, math.log(0.25)) and abs(r.entropy - 2 * LN2) < 1e-12
    free = row_of([0.45, 0.2, 0.1, 0.0, 0.1, 0.05, 0.05, 0.05])
    r = A.alternatives_np(free, 3, rng=(0, 4, 4, 8))
    assert r.gap < 0 and r.ids.tolist() == [0, 1, 2] and r.size == 7 and abs(r.logprobs[0] - math.log(0.45)) < 1e-12
    # a narrowed timestamp range and a suppressed timestamp leave A smaller, and the normaliser follows
    r = A.alternatives_np(free, 8, suppress=[4], rng=(0, 2, 5, 7))
    assert r.ids.tolist() == [0, 1, 5, 6] and abs(np.exp(r.logprobs).sum() - 1.0) < 1e-12
    # timestamps only (the first token): forced whatever the values
    r = A.alternatives_np(free, 2, rng=(0, 0, 4, 8))
    assert r.gap == np.inf and r.ids.tolist() == [4, 5]
    # text only (a closed pair)
    r = A.alternatives_np(free, 2, rng=(0, 4, 6, 6))
    assert r.gap == -np.inf and r.ids.tolist() == [0, 1]


@pytest.mark.parametrize("V,n,rows", A.SHAPES)
def test_the_seeded_rows_agree_with_the_beam_tests_restatement_and_keep_their_gap(V, n, rows):
    """The rows of the kernel test: the two f64 restatements list the same ids and log-probs, every feature of the recipe is
    there, and no row's sum-rule gap is below alt_ref.MIN_SUM_RULE_GAP -- so the GPU test skips no row."""
    s = A.seeded_rows(V, rows)
    assert A.min_sum_rule_gap(s) >= A.MIN_SUM_RULE_GAP
    if (V, n, rows) == (1024, 8, 128):
        assert abs(A.min_sum_rule_gap(s) - 0.0427) < 1e-4          # the smallest of all shapes
    assert np.isinf(s.logits[0]).sum() >= 15 and s.suppress.size >= 50
    for ts_on in (False, True):
        lg, rng = A.case_inputs(s, ts_on)
        ref = A.case_reference(s, n, ts_on)
        other = _lists_np(lg, n - 1, s.suppress, rng)
        for b, (r, (top, lp, gap, _)) in enumerate(zip(ref, other)):
            assert r.ids.tolist() == top.tolist() and np.allclose(r.logprobs, lp, rtol=0, atol=1e-12), (b, ts_on)
            assert r.count == min(n, r.size) and r.entropy > 0
            assert not set(r.ids.tolist()) & set(s.suppress.tolist())
        if rows > 2:
            if not ts_on:                                                                    # row 1: a tie at the top
                tied = [int(i) for i in np.flatnonzero(lg[1] == lg[1].max()) if i not in set(s.suppress.tolist())]
                assert len(np.flatnonzero(lg[1] == lg[1].max())) == 3 and ref[1].ids[:len(tied)].tolist()[:n] == tied[:n]
            assert max(lg[2]) == 50.0 and lg[2][ref[2].ids[0]] < 50.0                        # row 2: the large ids are suppressed
        if ts_on:
            assert sum(1 for r in ref if r.gap > 0) >= 2 and sum(1 for r in ref if r.gap < 0) >= 1


# ---------------------------------------------------------------- the wrappers' packing on a stand-in library
class AltLib(FakeLib):
    """FakeLib plus wm_request_alternatives: the request is recorded by its fields, and the next recorded call fills its buffers
    -- ids 100 * row + 10 * position + entry, log-probs -(entry + 1) / 8, counts n, entropy position + row / 4."""

    def __init__(self):
        FakeLib.__init__(self)
        self.pending = None

        def request(h, req):
            if req is None:
                self.calls.append(["wm_request_alternatives", None])
                self.pending = None
                return B.WM_OK
            r = req._obj
            self.calls.append(["wm_request_alternatives", dict(n=r.n, rows=r.rows, max_new=r.max_new, tokens=bool(r.tokens),
                                                               logprobs=bool(r.logprobs), counts=bool(r.counts),
                                                               entropy=bool(r.entropy))])
            self.pending = (r.n, r.rows, r.max_new, r.tokens, r.logprobs, r.counts, r.entropy)
            return B.WM_OK
        self.wm_request_alternatives = request

    def _record(self, name, args):
        st = FakeLib._record(self, name, args)
        if self.pending is not None and name.startswith("wm_transcribe"):
            n, rows, max_new, tok, lp, cnt, ent = self.pending
            self.pending = None
            r, p, j = np.meshgrid(np.arange(rows), np.arange(max_new), np.arange(n), indexing="ij")
            _at(tok, "int32", (rows, max_new, n))[...] = 100 * r + 10 * p + j
            _at(lp, "float32", (rows, max_new, n))[...] = -(j + 1) / 8.0
            if cnt:
                _at(cnt, "int32", (rows, max_new))[...] = n
            if ent:
                _at(ent, "float32", (rows, max_new))[...] = p[..., 0] + r[..., 0] / 4.0
        return st


def alt_ctx():
    c = object.__new__(B.Context)
    c.lib, c.handle = AltLib(), ctypes.c_void_p(0xC0DE)
    c.dims = dict(n_mels=80, n_text_ctx=64, n_vocab=128)
    c.lib.blob = ("float32", (MEL.size,))
    return c


def names(ctx):
    return [c[0] for c in ctx.lib.calls]


def test_request_alternatives_packs_the_struct_and_keeps_the_arrays():
    c = alt_ctx()
    a = c.request_alternatives(5, 6, 4)
    assert c.lib.calls == [["wm_request_alternatives", dict(n=5, rows=6, max_new=4, tokens=True, logprobs=True, counts=True,
                                                            entropy=True)]]
    assert a.tokens.shape == (6, 4, 5) and a.tokens.dtype == np.int32 and np.all(a.tokens == -1)
    assert a.logprobs.shape == (6, 4, 5) and a.logprobs.dtype == np.float32 and a.counts.shape == (6, 4) and a.entropy.shape == (6, 4)
    assert c.lib.wm_request_alternatives.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    assert c.lib.wm_request_alternatives.restype is ctypes.c_int
    assert c.lib.pending[3] == a.tokens.ctypes.data and c.lib.pending[4] == a.logprobs.ctypes.data
    assert c.lib.pending[5] == a.counts.ctypes.data and c.lib.pending[6] == a.entropy.ctypes.data
    assert c._alt_request[0] is a                                         # kept alive until the next request
    b2 = c.request_alternatives(1, 2, 3, entropy=False)
    assert b2.entropy is None and c.lib.calls[-1][1]["entropy"] is False
    assert c.request_alternatives(None, 0, 0) is None and c.lib.calls[-1] == ["wm_request_alternatives", None]
    assert ctypes.sizeof(B.wm_alternatives_out) == 56                      # i32, pad, i64, i32, pad, four pointers


def test_every_wrapper_requests_right_in_front_of_its_call_and_packs_the_result():
    win = (MEL, BASE3, LEN3, SEEK3, NF3)

    def windows(c):
        c.lib.n_windows = 3
        return B.Windows(c, ctypes.c_void_p(SET_HANDLE), np.arange(3, dtype=np.int32) + 2)
    plain = {
        "wm_transcribe_mel": lambda c, **kw: c.transcribe_mel(*win, P3, 4, eot=50, **kw),
        "wm_transcribe_mel_ragged": lambda c, **kw: c.transcribe_mel(*win, RAGGED, 4, eot=50, sot_tail=3, budgets=[4, 3, 2], **kw),
        "wm_transcribe_windows": lambda c, **kw: c.transcribe_windows(windows(c), None, P3, 4, eot=50, **kw),
    }
    for entry, call in plain.items():
        c0, c1 = alt_ctx(), alt_ctx()
        r0, r1 = call(c0), call(c1, alternatives=2)
        assert "wm_request_alternatives" not in names(c0) and r0.alt_tokens is None and r0.entropy is None
        assert names(c1)[-2:] == ["wm_request_alternatives", entry]
        assert [x for x in c1.lib.calls if x[0] != "wm_request_alternatives"] == c0.lib.calls, entry     # nothing else moves
        assert c1.lib.calls[-2][1] == dict(n=2, rows=3, max_new=4, tokens=True, logprobs=True, counts=True, entropy=True)
        assert r1.alt_tokens.shape == (3, 4, 2) and r1.alt_tokens[2, 3].tolist() == [230, 231]
        assert r1.alt_logprobs[1, 0].tolist() == [-0.125, -0.25] and np.all(r1.alt_counts == 2) and r1.entropy[2, 3] == 3.5
        assert np.array_equal(r1.tokens, r0.tokens)
    # best-of: rows = B * best_of, results [B][N]..., and `selected` carries the chosen candidate's
    best = {
        "wm_transcribe_mel_best_of": lambda c, **kw: c.transcribe_mel_best_of(*win, P3, 4, 2, eot=50, temperature=0.5, **kw),
        "wm_transcribe_windows": lambda c, **kw: c.transcribe_windows_best_of(windows(c), None, P3, 4, 2, eot=50, temperature=0.5, **kw),
    }
    for entry, call in best.items():
        c0, c1 = alt_ctx(), alt_ctx()
        r0, r1 = call(c0), call(c1, alternatives=3, budgets=[1, 2, 3])
        assert names(c1)[-2] == "wm_request_alternatives" and c1.lib.calls[-2][1]["rows"] == 6
        assert names(c1)[0] == "wm_set_token_budgets"                         # the request is the LAST thing in front of the call
        assert r0.alt_tokens is None and r0.selected.alt_tokens is None
        assert r1.alt_tokens.shape == (3, 2, 4, 3) and r1.alt_counts.shape == (3, 2, 4) and r1.entropy.shape == (3, 2, 4)
        assert r1.alt_tokens[2, 1, 0].tolist() == [500, 501, 502]              # hypothesis row 2 * 2 + 1
        rows = np.arange(3)
        assert np.array_equal(r1.selected.alt_tokens, r1.alt_tokens[rows, r1.best]) and r1.selected.alt_tokens.shape == (3, 4, 3)
        assert np.array_equal(r1.selected.entropy, r1.entropy[rows, r1.best]) and r1.best.tolist() == [0, 1, 0]
    # the entries of transcribe_mel: best_of goes through the best-of wrapper and returns its `selected`
    c = alt_ctx()
    r = c.transcribe_mel(*win, P3, 4, eot=50, temperature=0.5, best_of=2, alternatives=3)
    assert names(c)[-2:] == ["wm_request_alternatives", "wm_transcribe_mel_best_of"] and r.alt_tokens.shape == (3, 4, 3)
    assert r.alt_tokens[1, 0].tolist() == [300, 301, 302]                      # candidate 1 of row 1
    # (the stand-in has no signature for wm_transcribe and the *_aligned entries: those wrappers run in tests/test_alternatives_gpu.py)


BAD = [0, 17, -1, 2.5, True, "3", np.float32(4.0)]


def test_bad_values_raise_before_any_library_call():
    assert B.alternatives_arg(None) is None and B.alternatives_arg(np.int64(16)) == 16 and B.alternatives_arg(1) == 1
    for v in BAD:
        with pytest.raises(ValueError):
            B.alternatives_arg(v)
    with pytest.raises(ValueError):
        B.alternatives_arg(3, beam_size=2)
    with pytest.raises(ValueError):
        B.alternatives_arg(3, draft=object())
    assert B.alternatives_arg(None, beam_size=2, draft=object()) is None        # no request: nothing to refuse
    win = (MEL, BASE3, LEN3, SEEK3, NF3)
    for v in BAD:
        c = alt_ctx()
        for call in (lambda: c.transcribe_mel(*win, P3, 4, eot=50, alternatives=v, budgets=[1, 1, 1]),
                     lambda: c.transcribe_mel_best_of(*win, P3, 4, 2, eot=50, alternatives=v, budgets=[1, 1, 1]),
                     lambda: c.transcribe_mel_raw(*win, P3, 4, 50, alternatives=v, budgets=[1, 1, 1])):
            with pytest.raises(ValueError):
                call()
        assert c.lib.calls == []
    c = alt_ctx()
    for kw in (dict(beam_size=2), dict(beam_size=2, patience=1.5)):
        with pytest.raises(ValueError, match="beam"):
            c.transcribe_mel(*win, P3, 4, eot=50, alternatives=3, **kw)
    assert c.lib.calls == []

    class Never:
        dims = dict(n_vocab=1024, n_mels=80, n_text_ctx=448)

        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    for kw in [dict(alternatives=v) for v in BAD] + [dict(alternatives=3, beam_size=2)]:
        with pytest.raises(ValueError):
            B.transcribe_with_fallback(Never(), np.zeros((1, 16), np.float32), [1], 4, 5, **kw)


def fake_result(n_rows, max_new, t, n_alt, eot=63):
    """a TranscribeResult whose values name the attempt: log-probs t - 1.1 (better with every step), alternatives' ids 1000 t"""
    toks = np.tile(np.arange(max_new, dtype=np.int32), (n_rows, 1))
    r = B.TranscribeResult(toks, np.full(n_rows, max_new, np.int32), np.full((n_rows, max_new), t - 1.1, np.float32), None, eot)
    if n_alt:
        a = B.Alternatives(n_alt, n_rows, max_new)
        a.tokens[...] = int(1000 * t)
        a.logprobs[...] = -t
        a.counts[...] = n_alt
        a.entropy[...] = t
        a.attach(r)
    return r


def test_transcribe_with_fallback_requests_in_front_of_every_attempt_and_keeps_the_kept_attempts_values():
    calls = []

    class Ctx:
        dims = dict(n_vocab=64, n_mels=80, n_text_ctx=448)

        def transcribe(self, pcm, prompt, max_new, **kw):
            calls.append(("transcribe", kw["temperature"], kw.get("alternatives")))
            return fake_result(len(pcm), max_new, kw["temperature"], kw.get("alternatives"))
    pcm = np.zeros((3, 16), np.float32)
    out = B.transcribe_with_fallback(Ctx(), pcm, [1], 4, 63, temperatures=(0.0, 0.5, 1.0), logprob_threshold=-0.7)
    assert [c[1:] for c in calls] == [(0.0, None), (0.5, None)] and "alt_tokens" not in out and "entropy" not in out
    del calls[:]
    # avg_logprob = (t - 1.1) * 4 / 5 = -0.88, -0.48, -0.08: the attempts at 0 and 0.5 fail the bar of -0.3, the one at 1 is kept
    out = B.transcribe_with_fallback(Ctx(), pcm, [1], 4, 63, temperatures=(0.0, 0.5, 1.0), logprob_threshold=-0.3,
                                     compression_ratio_threshold=None, alternatives=2)
    assert calls == [("transcribe", 0.0, 2), ("transcribe", 0.5, 2), ("transcribe", 1.0, 2)]
    assert out["alt_tokens"].shape == (3, 4, 2) and np.all(out["alt_tokens"] == 1000) and np.all(out["entropy"] == 1.0)
    assert np.all(out["alt_logprobs"] == -1.0) and np.all(out["alt_counts"] == 2) and np.all(out["temperature"] == 1.0)


# ---------------------------------------------------------------- transcribe_long on the recording fake
class AltCtx(RecCtx):
    """RecCtx whose decode entries serve alternatives=: per token the list [(token, -t - 0.125), (token + 1, -t - 0.25), ...]
    and the entropy position + t -- so that a segment's values name the position and the attempt they came from."""

    def _decode(self, ids, max_new, kw):
        r = RecCtx._decode(self, ids, max_new, kw)
        n = kw.get("alternatives")
        if n:
            a = B.Alternatives(n, len(ids), max_new)
            t = kw["temperature"]
            for i in range(len(ids)):
                for p in range(int(r.lens[i])):
                    a.tokens[i, p] = r.tokens[i, p] + np.arange(n)
                    a.logprobs[i, p] = -t - 0.125 * (np.arange(n) + 1)
                    a.counts[i, p] = n
                    a.entropy[i, p] = p + t
            a.attach(r)
        return r


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def _run(case, **extra):
    ctx = AltCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    got = dict(calls=ctx.calls)
    try:
        got["out"] = canon(B.transcribe_long(ctx, recs, **dict(case["kw"], **extra)))
    except (ValueError, RuntimeError) as e:
        got["error"] = [type(e).__name__, str(e)]
    return got


def _case_names():
    plain = [n for n in sorted(cases(None)) if not n.startswith("error_")]
    return sorted(set(plain[::5] + [n for n in plain if n.startswith("decode_raises")]))


def _refused(kw):
    return any(kw.get(k) is not None for k in ("beam_size", "patience", "draft"))


def _strip(out):
    """the result without the two per-segment keys"""
    out = [dict(rec, segments=[{k: v for k, v in sg.items() if k not in ("token_alternatives", "token_entropy")}
                               for sg in rec["segments"]]) for rec in out]
    return out


@pytest.mark.parametrize("name", _case_names())
def test_transcribe_long_requests_in_front_of_every_decode_call(vocab, name):
    """alternatives=None: the plain run's call log.  alternatives=3: the same log with alternatives=3 on EVERY decode call (the
    wrapper turns it into one wm_request_alternatives right in front of its C call: the test above), the same result, and every
    segment carries the kept attempt's values of its own tokens.  With beam_size or a draft: ValueError before any call."""
    case = cases(vocab)[name]
    plain = run_case(case)
    none = _run(case, alternatives=None)
    assert canon(none["calls"]) == plain["calls"]
    got = _run(case, alternatives=3)
    if _refused(case["kw"]):
        assert got["error"][0] == "ValueError" and not [c for c in got["calls"] if c[0] != "__init__"]
        return
    calls = canon(got["calls"])
    decodes = [c for c in calls if c[0].startswith("transcribe_")]
    assert decodes and all(["alternatives", 3] in c[2] for c in decodes)
    assert [[c[0], c[1], [kv for kv in c[2] if kv[0] != "alternatives"]] for c in calls] == plain["calls"]
    assert ("error" in got) == ("error" in plain)
    if "error" in plain:
        return
    assert _strip(got["out"]) == plain["out"]
    n_tok = 0
    for rec in got["out"]:
        for sg in rec["segments"]:
            alts, ent = sg["token_alternatives"], sg["token_entropy"]
            assert len(alts) == len(sg["tokens"]) == len(ent)
            for tok, alt, h in zip(sg["tokens"], alts, ent):
                t = sg["temperature"]
                assert [a[0] for a in alt] == [tok, tok + 1, tok + 2]
                assert np.allclose([a[1] for a in alt], [-t - 0.125, -t - 0.25, -t - 0.375])       # the KEPT attempt's
                assert abs((h - t) - round(h - t)) < 1e-6
                n_tok += 1
            if len(ent) > 1:       # consecutive positions of the window, in order
                assert np.allclose(np.diff(ent), 1.0)
    assert n_tok > 0


def test_bad_values_raise_before_transcribe_longs_first_call(vocab):
    name = [n for n in sorted(cases(vocab)) if not n.startswith(("error_", "decode_raises")) and not _refused(cases(vocab)[n]["kw"])][0]
    case = cases(vocab)[name]
    for v in BAD:
        got = _run(case, alternatives=v)
        assert got["error"][0] == "ValueError" and not [c for c in got["calls"] if c[0] != "__init__"], v
    for kw in (dict(beam_size=2), dict(draft=object())):
        got = _run(case, alternatives=3, **kw)
        assert got["error"][0] == "ValueError" and not [c for c in got["calls"] if c[0] != "__init__"], kw


def test_window_segments_slices_the_alternatives_with_the_tokens():
    ts = 100
    toks = [ts, 5, 6, ts + 10, ts + 10, 7, ts + 20]
    alts = [[(t, -0.5)] for t in toks]
    ent = [float(i) for i in range(len(toks))]
    res = dict(temperature=0.0, avg_logprob=-0.1, compression_ratio=1.0, no_speech_prob=0.0)
    segs, _ = B.window_segments(toks, 0, 3000, ts, 200, res, alternatives=(alts, ent))
    assert [sg["tokens"] for sg in segs] == [toks[:4], toks[4:]]
    assert [sg["token_entropy"] for sg in segs] == [ent[:4], ent[4:]]
    assert [[a[0][0] for a in sg["token_alternatives"]] for sg in segs] == [toks[:4], toks[4:]]
    plain, _ = B.window_segments(toks, 0, 3000, ts, 200, res)
    assert all("token_alternatives" not in sg and "token_entropy" not in sg for sg in plain)
    # a cleared segment loses them with its tokens
    segs, _ = B.window_segments([ts, ts + 5, ts + 5, 9, ts + 9], 0, 3000, ts, 200, res, alternatives=([[(1, 0.0)]] * 5, [0.0] * 5))
    assert len(segs) == 3      # [ts, ts + 5] and [ts + 5] are text-less, [ts + 5, 9, ts + 9] stays
    for sg in segs[:2]:
        assert sg["tokens"] == [] and sg["token_alternatives"] == [] and sg["token_entropy"] == []
    assert segs[2]["tokens"] == [ts + 5, 9, ts + 9] and len(segs[2]["token_alternatives"]) == 3 and len(segs[2]["token_entropy"]) == 3
