"""The sampling rules (wm_set_sampling_rules) without a device: the numpy restatement
(tests/sampling_ref.py) against a torch restatement of Hugging Face's three warpers, the wrapper's packing and its ValueErrors
against a stand-in library, transcribe_long's calls on the recording fake of test_longform_calls_cpu.py, and the cap on the
share of near-threshold rows among the inputs of tests/test_sampling_rules_kernel_gpu.py."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import sampling_ref as S
from test_longform_calls_cpu import RecCtx, SECONDS, canon, cases, make_vocab, run_case
from test_longform_clips_cpu import _rec

B = importlib.import_module("openai_whisper_coreml_amd.binding")


# ---------------------------------------------------------------- Hugging Face's warpers, written out (sort-based, f64)
def hf_warp(scores, T, top_k, top_p, min_p):
    """TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper in generate's order; returns the kept mask.
    scores: f64 tensor with -inf at the ids outside the admissible set."""
    s = scores / T
    if top_k > 0:
        k = min(top_k, s.numel())
        s = s.masked_fill(s < torch.topk(s, k)[0][-1], float("-inf"))            # (keeps every id tied with the k-th)
    if top_p < 1.0:
        sv, si = torch.sort(s, descending=False)
        cum = sv.softmax(-1).cumsum(-1)
        rm = cum <= (1 - top_p)
        rm[-1:] = False                                                          # min_tokens_to_keep = 1
        s = s.masked_fill(rm.scatter(0, si, rm), float("-inf"))
    if min_p > 0.0:
        p = s.softmax(-1)
        sv, si = torch.sort(s, descending=True)
        rm = (p < min_p * p.max())[si]
        rm[:1] = False
        s = s.masked_fill(rm.scatter(0, si, rm), float("-inf"))
    return torch.isfinite(s).numpy()


RULE_SETS = [(1, 1.0, 0.0), (8, 1.0, 0.0), (50, 1.0, 0.0), (2000, 1.0, 0.0), (0, 0.5, 0.0), (0, 0.9, 0.0), (0, 0.999, 0.0),
             (0, 1.0, 0.05), (0, 1.0, 0.5), (50, 0.9, 0.05), (8, 0.5, 0.3)]


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_the_restatement_keeps_what_hugging_faces_warpers_keep(T):
    """Rows without a tie at the cut and away from a threshold: the two kept sets are equal."""
    g = np.random.default_rng(int(T * 10))
    checked = 0
    for trial in range(60):
        V = int(g.choice([16, 300, 1024]))
        v = (g.standard_normal(V) * g.choice([1.0, 4.0, 8.0])).astype(np.float32)
        adm = g.random(V) < 0.8
        adm[int(g.integers(V))] = True
        inv_T = float(np.float32(1.0 / T))
        for rule in RULE_SETS:
            d = S.kept_detail(v, adm, inv_T, *rule)
            if d.tie or d.slack <= S.TOL:
                continue
            s = torch.from_numpy(np.where(adm, v.astype(np.float64), -np.inf))
            want = hf_warp(s, 1.0 / inv_T, *rule)
            got = np.zeros(V, bool)
            got[d.ids[:d.count]] = True
            assert np.array_equal(got, want), (trial, rule, d.count, int(want.sum()))
            ids, count, slack = S.kept(v, adm, inv_T, *rule)
            assert count == d.count and np.array_equal(ids, d.ids) and slack == d.slack
            checked += 1
    assert checked >= 500, checked


def test_top_k_keeps_exactly_k_where_hugging_face_keeps_the_ties():
    """The stated difference: values 5, 4, 4, 4, 1 under top_k = 2 -- Hugging Face keeps all three 4s, the rules here keep the
    lowest tied id only.  And -inf is never kept, whatever k says."""
    v = np.array([4, 5, 4, 1, 4], np.float32)
    adm = np.ones(5, bool)
    d = S.kept_detail(v, adm, 1.0, 2, 1.0, 0.0)
    assert d.count == 2 and d.ids[:2].tolist() == [1, 0] and d.tie
    assert np.flatnonzero(hf_warp(torch.from_numpy(v.astype(np.float64)), 1.0, 2, 1.0, 0.0)).tolist() == [0, 1, 2, 4]
    v2 = np.array([-np.inf, 2, -np.inf, 1], np.float32)
    assert S.kept(v2, adm[:4], 1.0, 4)[1] == 2 and S.kept(v2, np.array([1, 0, 1, 0], bool), 1.0, 4)[1] == 0
    # never fewer than one id; top_p over what top_k left
    assert S.kept(v, adm, 1.0, 0, 1e-6, 0.0)[1] == 1 and S.kept(v, adm, 1.0, 0, 1.0, 0.999)[1] == 1
    e = np.exp([0.0, -1.0, -1.0, -1.0, -4.0])
    assert S.kept(v, adm, 1.0, 3, 0.7, 0.0)[1] == (2 if (e[0] + e[1]) / e[:3].sum() >= 0.7 else 3)


# ---------------------------------------------------------------- the kernel test's inputs: the cap
def test_at_most_five_percent_of_the_kernel_tests_rows_are_inside_the_slack():
    """Over EXACTLY the (row, rule) cases the GPU kernel test checks (sampling_ref.checked_cases: the whole pool under the
    thirteen rule sets, 17 rows at T = 2 and without timestamp rules) with a top_p or min_p rule, not counting rows whose cut
    falls among ties: at most 5 % may be near a threshold (slack <= 1e-4), where the test accepts more than one count -- per
    vocabulary.  Also: no row's sum rule is near its tie (the reference decides `forced` in f64, the kernel from f32 partials)."""
    for V in S.GEOM:
        inp = S.hook_inputs(V)
        cache = {}
        near = total = 0
        for T, with_rng, rule, rows in S.checked_cases(V):
            ref = S.case_reference(inp, T, with_rng, rule, rows, cache)
            if rule[1] < 1.0 or rule[2] > 0.0:
                for d in ref:
                    if d.count and not d.tie:
                        total += 1
                        near += d.slack <= S.TOL
        print("V %d: %d of %d checked non-tie cases inside the slack" % (V, near, total))
        assert total >= 700 and near <= 0.05 * total, (V, near, total)
        sets, ref = S.pool_reference(inp, 1.0, S.rules_for(V))
        assert min(abs(s[2]) for s in sets if np.isfinite(s[2])) > 1e-3
        kinds = {k: [r for r in range(S.POOL_ROWS) if inp.kinds[r] == k] for k in S.KINDS}
        assert all(len(v) == 16 for v in kinds.values())
        assert all(ref[(1, 1.0, 0.0)][r].count == 0 for r in kinds["none"])
        assert all(len(ref[(1, 1.0, 0.0)][r].ids) == 1 for r in kinds["one"])
        assert all(sets[r][1] for r in kinds["forced"])
        k50 = ref[(50, 1.0, 0.0)]
        assert all(k50[r].count < min(50, V) for r in kinds["cut_inf"])            # -inf ids at the cut: fewer than k are kept
        if V > 16:
            assert all(k50[r].tie for r in kinds["equal"])
        assert {inp.kinds[r] for r in S.SUB17} == set(S.KINDS)


# ---------------------------------------------------------------- the wrapper's packing
class StandIn:
    def __init__(self, status=0):
        self.calls, self.status = [], status

        def fn(*a):
            self.calls.append(a)
            return self.status
        self.wm_set_sampling_rules = fn

    def wm_last_error(self):
        return b"stand-in"


def _ctx(lib):
    c = object.__new__(B.Context)
    c.lib, c.handle = lib, ctypes.c_void_p(0x1234)
    return c


def test_the_wrapper_packs_top_k_top_p_and_min_p():
    lib = StandIn()
    c = _ctx(lib)
    c.set_sampling_rules(50, 0.9, 0.05)
    c.set_sampling_rules(top_k=np.int64(8))
    c.set_sampling_rules(top_p=np.float32(0.5), min_p=0.25)
    c.set_sampling_rules()
    assert [a[1:] for a in lib.calls] == [(50, 0.9, 0.05), (8, 1.0, 0.0), (0, 0.5, 0.25), (0, 1.0, 0.0)]
    assert all(a[0] is c.handle and type(a[1]) is int and type(a[2]) is float and type(a[3]) is float for a in lib.calls)
    assert lib.wm_set_sampling_rules.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    assert lib.wm_set_sampling_rules.restype is ctypes.c_int
    with pytest.raises(B.WhisperError):
        _ctx(StandIn(status=1)).set_sampling_rules(-1)


BAD = [dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1),
       dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=float("nan")), dict(top_k=5, min_p=2.0)]


def test_the_keyword_arguments_are_checked_before_any_library_call():
    assert B.sampling_rules_args() is None and B.sampling_rules_args(None, None, None) is None
    assert B.sampling_rules_args(top_k=np.int32(50)) == (50, 1.0, 0.0) and B.sampling_rules_args(0, 1.0, 0.0) == (0, 1.0, 0.0)
    assert B.sampling_rules_args(top_p=0.9, min_p=0.05) == (0, 0.9, 0.05)
    for kw in BAD:
        with pytest.raises(ValueError):
            B.sampling_rules_args(**kw)

    class Never:
        dims = dict(n_vocab=1024, n_mels=80, n_text_ctx=448)

        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    for kw in BAD:
        with pytest.raises(ValueError):
            B.transcribe_with_fallback(Never(), np.zeros((1, 16), np.float32), [1], 4, 5, **kw)


def test_transcribe_with_fallback_sets_the_rules_for_the_run_and_clears_them():
    calls = []

    class Ctx:
        dims = dict(n_vocab=64, n_mels=80, n_text_ctx=448)

        def set_sampling_rules(self, *a):
            calls.append(("set",) + a)

        def transcribe(self, pcm, prompt, max_new, **kw):
            calls.append(("transcribe", kw["temperature"]))
            if self.fail:
                raise RuntimeError("decode")
            n = len(pcm)
            toks = np.tile(np.arange(max_new, dtype=np.int32), (n, 1))
            return B.TranscribeResult(toks, np.full(n, max_new, np.int32), np.full((n, max_new), -0.1, np.float32), None, 63)
    ctx = Ctx()
    ctx.fail = False
    B.transcribe_with_fallback(ctx, np.zeros((2, 16), np.float32), [1], 4, 63, temperatures=(0.0, 0.5))
    assert [c[0] for c in calls] == ["transcribe"]                     # all None: the calls made today
    del calls[:]
    B.transcribe_with_fallback(ctx, np.zeros((2, 16), np.float32), [1], 4, 63, temperatures=(0.0, 0.5), top_k=50, top_p=0.9)
    assert calls[0] == ("set", 50, 0.9, 0.0) and calls[-1] == ("set",) and [c[0] for c in calls[1:-1]] == ["transcribe"]
    del calls[:]
    ctx.fail = True
    with pytest.raises(RuntimeError):
        B.transcribe_with_fallback(ctx, np.zeros((2, 16), np.float32), [1], 4, 63, min_p=0.1)
    assert calls[0] == ("set", 0, 1.0, 0.1) and calls[-1] == ("set",)


# ---------------------------------------------------------------- transcribe_long on the recording fake
class RulesCtx(RecCtx):
    def set_sampling_rules(self, *a, **kw):
        self._log("set_sampling_rules", a, kw)


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def _run(case, **extra):
    ctx = RulesCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    got = dict(calls=ctx.calls)
    try:
        got["out"] = canon(B.transcribe_long(ctx, recs, **dict(case["kw"], **extra)))
    except (ValueError, RuntimeError) as e:
        got["error"] = [type(e).__name__, str(e)]
    return got


def _case_names():
    names = sorted(cases(None))
    plain = [n for n in names if not n.startswith("error_")]
    return plain[::7] + [n for n in plain if n.startswith("decode_raises")]


@pytest.mark.parametrize("name", sorted(set(_case_names())))
def test_transcribe_long_sets_the_rules_once_and_clears_them(vocab, name):
    """With the keywords the call log is the plain run's plus ONE set call (behind the log-mel, in front of every decode) and
    ONE clear call at the very end -- also when a decode raises; with all three None it is the plain run's log."""
    case = cases(vocab)[name]
    plain = run_case(case)
    none = _run(case, top_k=None, top_p=None, min_p=None)
    assert canon(none["calls"]) == plain["calls"]
    for kw, want in ((dict(top_k=50, top_p=0.9, min_p=0.05), [50, 0.9, 0.05]), (dict(top_k=8), [8, 1.0, 0.0]),
                     (dict(top_p=0.5), [0, 0.5, 0.0]), (dict(min_p=0.25), [0, 1.0, 0.25])):
        got = _run(case, **kw)
        assert ("error" in got) == ("error" in plain)
        if "error" in plain:
            assert got["error"] == plain["error"]
        else:
            assert got["out"] == plain["out"]
        calls = canon(got["calls"])
        at = [i for i, c in enumerate(calls) if c[0] == "set_sampling_rules"]
        assert len(at) == 2 and at[1] == len(calls) - 1, [c[0] for c in calls]
        assert calls[at[0]] == ["set_sampling_rules", want, []] and calls[at[1]] == ["set_sampling_rules", [], []]
        assert [c for i, c in enumerate(calls) if i not in at] == plain["calls"]
        names = [c[0] for c in calls]
        mel = max(i for i, n_ in enumerate(names) if n_ in ("logmel_long", "logmel_long_device"))
        first_use = min(i for i, n_ in enumerate(names) if n_.startswith(("transcribe_", "encode_windows", "windows_detect")))
        assert mel < at[0] < first_use


def test_the_rules_go_behind_the_sequence_bias_and_bad_values_raise_first(vocab):
    assert any(n.startswith("decode_raises") for n in _case_names())
    got = _run(cases(vocab)["decode_raises_in_a_reuse_round"], top_k=3)
    assert got["error"][0] == "RuntimeError" and got["calls"][-1][0] == "set_sampling_rules"
    name = [n for n in sorted(cases(vocab)) if not n.startswith(("error_", "decode_raises"))][0]
    case = cases(vocab)[name]

    class Both(RulesCtx):
        def set_sequence_bias(self, *a, **kw):
            self._log("set_sequence_bias", (), {})

        def set_repetition_rules(self, *a, **kw):
            self._log("set_repetition_rules", (), {})
    ctx = Both(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    B.transcribe_long(ctx, recs, **dict(case["kw"], top_k=5, bad_words=[[3]], no_repeat_ngram_size=2))
    names = [c[0] for c in ctx.calls if c[0].startswith("set_s") or c[0] == "set_repetition_rules"]
    assert names == ["set_repetition_rules", "set_sequence_bias", "set_sampling_rules", "set_sampling_rules", "set_sequence_bias",
                     "set_repetition_rules"], names
    for kw in BAD:
        got = _run(case, **kw)
        assert got["error"][0] == "ValueError" and not [c for c in got["calls"] if c[0] != "__init__"], (kw, got.get("calls"))
