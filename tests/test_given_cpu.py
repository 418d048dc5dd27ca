"""CPU tests of given tokens (wm_set_given_tokens): the f64 restatement of tests/given_ref.py on
hand-worked rows, the seeded rows' distance from a sum-rule tie, the pending bit and every refusal message (the CPU route of
tests/test_pending_cpu.py), the group's table (wm_group_given through wmdbg_group_given), and the wrappers of binding.py on a
stand-in library: packing, "armed right in front of the C call", the ValueErrors and score_given's two call shapes.  With
given=None the wrappers' and transcribe_long's call logs are the parent goldens."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import alt_ref as A
import given_ref as G
import test_binding_calls_cpu as BC
import test_longform_calls_cpu as LC
from test_alternatives_cpu import AltLib
from test_binding_calls_cpu import BASE3, LEN3, MEL, NF3, P3, RAGGED, SEEK3, SET_HANDLE, _at
from test_pending_cpu import KINDS, WM_ERR_STATE, WM_OK, answer, lib   # noqa: F401 (lib: fixture)

B = importlib.import_module("openai_whisper_coreml_amd.binding")
GIVEN = 32   # WM_PEND_GIVEN
ALT, SAMP_ROWS = 16, 8


# ---------------------------------------------------------------- the restatement by hand
def row(text_p, ts_p):
    """logits = log(weight): ids 0 .. 4 text (eot = 4), ids 5 .. 7 timestamps"""
    with np.errstate(divide="ignore"):
        return np.log(np.array(list(text_p) + list(ts_p), np.float64))


TEXT = (1, 2, 4, 0, 1)          # id 3 has v = -inf; the best text weighs 4
FREE, FORCING = (1, 1, 1), (4, 2, 2)   # timestamps summing to 3 < 4 (not forced) and to 8 > 4 (forced)
RNG = (0, 5, 5, 8)


def lp_of(v, tok, suppress=(), rng=RNG):
    return G.given_np(v, tok, suppress, rng, 5)


def test_the_nine_cases_by_hand():
    free, forcing = row(TEXT, FREE), row(TEXT, FORCING)
    seen = {}
    # (row, id, ranges, log-prob, forced)
    for v, tok, rng, want, forced in [
            (free, 2, RNG, math.log(4 / 11), False),              # admissible text, rule not forcing: over text + timestamps
            (forcing, 2, RNG, -np.inf, True),                     # admissible text, rule forcing: the rule excludes it
            (free, 5, RNG, math.log(1 / 11), False),              # admissible timestamp, rule not forcing
            (forcing, 5, RNG, math.log(4 / 8), True),             # admissible timestamp, rule forcing: over the timestamps alone
            (free, 3, RNG, -np.inf, False),                       # inadmissible text (v = -inf), rule not forcing
            (forcing, 3, RNG, -np.inf, True),                     # inadmissible text, rule forcing
            (free, 5, (0, 5, 6, 8), -np.inf, False),              # inadmissible timestamp (below the range): 2 < 4, not forcing
            (forcing, 5, (0, 5, 6, 8), -np.inf, False),           # ... 2 + 2 = 4 is not above 4 either: still not forcing
            (row(TEXT, (4, 4, 4)), 5, (0, 5, 6, 8), -np.inf, True),   # inadmissible timestamp, rule forcing (8 > 4)
            (free, 7, None, math.log(1 / 11), False)]:            # timestamp rules off: every id that is not suppressed
        r = G.given_np(v, tok, (), rng, 5)
        assert r.touched and r.forced == forced, (tok, rng)
        assert r.logprob == want if want == -np.inf else abs(r.logprob - want) < 1e-12, (tok, rng, r.logprob, want)
        seen[r.case] = seen.get(r.case, 0) + 1
    assert sorted(seen) == sorted(G.CASES)


def test_suppressed_banned_minus_infinity_and_the_edge_ids():
    free = row(TEXT, FREE)
    # the largest logit suppressed: the best text is 2 < 3, so the rule forces; the suppressed id is -inf however large
    r = lp_of(free, 2, suppress=[2])
    assert r.logprob == -np.inf and r.forced and r.case == "inadmissible text, forced"
    assert abs(lp_of(free, 5, suppress=[2]).logprob - math.log(1 / 3)) < 1e-12
    # a banned id is a suppressed one of its row: the others' normaliser loses it
    assert lp_of(free, 1, suppress=[1]).logprob == -np.inf
    assert abs(lp_of(free, 2, suppress=[1]).logprob - math.log(4 / 9)) < 1e-12
    assert lp_of(free, 3).logprob == -np.inf                                      # v = -inf
    for tok in (0, 4, 7):                                                         # ids 0, eot and V - 1
        assert abs(lp_of(free, tok).logprob - math.log(1 / 11)) < 1e-12
        assert abs(G.given_np(free, tok, (), None, 5).logprob - math.log(1 / 11)) < 1e-12
    assert lp_of(free, 0, rng=(4, 5, 5, 8)).logprob == -np.inf                    # below the text range
    assert lp_of(free, 7, rng=(0, 5, 5, 7)).logprob == -np.inf                    # V - 1 past the timestamp range
    # nothing admissible: the row is left to the close's own path
    r = lp_of(free, 2, suppress=list(range(8)))
    assert not r.touched and r.logprob == -np.inf


def test_the_advance_of_the_timestamp_history():
    tsb, eot, V = 5, 4, 8
    h, r = G.ts_advance_np([0, 0, 1, -1], 6, tsb, eot, V)          # the first token, a timestamp: a pair "closed" (len < 2)
    assert (h, r) == ([1, 1, 0, 6], [0, 5, 7, 5])
    h, r = G.ts_advance_np(h, 1, tsb, eot, V)                      # text: timestamps from 7 on
    assert (h, r) == ([2, 0, 1, 6], [0, 5, 7, 8])
    h, r = G.ts_advance_np(h, 7, tsb, eot, V)                      # an opening timestamp: its partner or eot
    assert (h, r) == ([3, 1, 0, 7], [4, 5, 7, 8])


@pytest.mark.parametrize("V,rows", G.SHAPES)
def test_the_seeded_rows_keep_their_distance_from_a_tie(V, rows):
    """f32 and f64 agree on `forced` on every seeded row of the kernel test's shapes; and the restatement gives the log-prob the
    alternatives' restatement gives the same id"""
    s = A.seeded_rows(V, rows)
    assert A.min_sum_rule_gap(s) >= A.MIN_SUM_RULE_GAP
    for ts_on in (False, True):
        lg, rng = A.case_inputs(s, ts_on)
        for b in range(min(rows, 8)):
            r4 = None if rng is None else rng[b]
            alt = A.alternatives_np(lg[b], 3, s.suppress, r4)
            for tok, lp in zip(alt.ids, alt.logprobs):
                got = G.given_np(lg[b], int(tok), s.suppress, r4, s.ts_begin)
                assert got.admissible and abs(got.logprob - lp) < 1e-12
            assert G.given_np(lg[b], int(s.suppress[0]), s.suppress, r4, s.ts_begin).logprob == -np.inf


# ---------------------------------------------------------------- the pending bit and the refusals
GIVEN_GREEDY = "wm_transcribe_greedy takes no given tokens (wm_set_given_tokens): it has no log-prob output"
GIVEN_BEAM = "beam-search calls take no given tokens (wm_set_given_tokens)"
GIVEN_HYP = "aligned best-of calls take no given tokens (wm_set_given_tokens)"
GIVEN_F32 = "given tokens are not supported by the all-f32 precision path"
GIVEN_SPEC = "speculative decoding takes no given tokens (wm_set_given_tokens)"
GIVEN_MULTI = "multi_transcribe_greedy takes no given tokens (wm_set_given_tokens)"
REFUSED = {
    "greedy": GIVEN_GREEDY, "plain": None, "mel, mel_aligned": None, "ragged, ragged aligned": None,
    "windows at one sample, windows_aligned": None, "windows at best_of 3": None, "mel_best_of at 1": None, "mel_best_of at 3": None,
    "windows_best_of_aligned at 1": GIVEN_HYP, "mel_beam": GIVEN_BEAM, "windows_beam at 1": GIVEN_BEAM, "mel_beam_aligned": GIVEN_BEAM,
    "speculative": GIVEN_SPEC, "multi": GIVEN_MULTI, "f32: mel": GIVEN_F32, "f32: greedy": GIVEN_GREEDY,
    "f32: windows at one sample": GIVEN_F32, "f32: mel_best_of": GIVEN_F32, "f32: mel_beam": GIVEN_BEAM,
}


def test_the_table_names_every_kind_of_call():
    assert sorted(REFUSED) == sorted(KINDS)


@pytest.mark.parametrize("name", list(KINDS))
def test_who_serves_given_tokens(lib, name):
    """the bit is 32; budgets and the two other row maps change no answer; alternatives are judged first, given tokens second,
    the sampling row map third; without the bit every answer is the one tests/test_pending_cpu.py pins"""
    kind, rows_msg, alt_msg = KINDS[name]
    msg = REFUSED[name]
    for low in range(32):
        want = (alt_msg if low & ALT else None) or msg or (rows_msg if low & SAMP_ROWS else None)
        assert answer(lib, GIVEN | low, kind) == ((WM_ERR_STATE, want) if want else (WM_OK, "")), (name, low)


def test_take_carries_the_table(lib):
    lib.wmdbg_pending_take.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    out = np.full(6, -7, dtype=np.int32)
    for bits, again in ((GIVEN, 0), (GIVEN | 1, GIVEN), (63, 63), (31, GIVEN)):
        assert lib.wmdbg_pending_take(bits, again, out.ctypes.data_as(ctypes.c_void_p)) == 0
        armed, taken, left, taken_later, member, _ = out.tolist()
        assert (armed, taken, left, taken_later, member) == (bits, bits, 0, bits, again)


# ---------------------------------------------------------------- the group's table
def test_group_tables(lib):
    fn = lib.wmdbg_group_given
    vp, ip = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, vp, ip, ip, ip, ip, ip, vp, vp, ip, vp]
    fn.restype = ip
    g = np.random.default_rng(11)
    for rows_call, N, stride in ((7, 1, 5), (4, 3, 6), (5, 2, 1)):
        n = rows_call * N
        lens = g.integers(0, stride + 1, n).astype(np.int32)
        lens[:N] = 0                                                   # window 0 decodes freely
        tok = g.integers(0, 1000, (n, stride)).astype(np.int32)
        for b0, Cg in ((0, 1), (0, rows_call), (1, rows_call - 1), (rows_call - 1, 1), (1, 2)):
            L, gl, gt = G.group_given_np(lens, tok, b0, Cg, N)
            lo, to, Lo = np.full(Cg * N, -7, np.int32), np.full(Cg * N * stride, -7, np.int32), np.full(1, -7, np.int32)
            st = fn(lens.ctypes.data, tok.ctypes.data, stride, n, b0, Cg, N, lo.ctypes.data, to.ctypes.data, to.size, Lo.ctypes.data)
            assert st == 0 and Lo[0] == L and np.array_equal(lo, gl)
            assert np.array_equal(to[:gt.size].reshape(gt.shape), gt) and np.all(to[gt.size:] == -7)
            assert (L == 0) == (b0 == 0 and Cg == 1)                   # (the seeds leave no other group without a given row)
    one = np.zeros(4, np.int32)
    assert fn(one.ctypes.data, one.ctypes.data, 1, 4, 3, 2, 1, one.ctypes.data, one.ctypes.data, 4, one.ctypes.data) != 0   # rows past the call
    assert fn(None, one.ctypes.data, 1, 4, 0, 1, 1, one.ctypes.data, one.ctypes.data, 4, one.ctypes.data) != 0


# ---------------------------------------------------------------- the wrappers on a stand-in library
class GivenLib(AltLib):
    """AltLib plus wm_set_given_tokens: the table is recorded as the arrays read back from the addresses"""

    def __init__(self):
        AltLib.__init__(self)

        def put(h, tokens, stride, lens, n):
            if n == 0:
                self.calls.append(["wm_set_given_tokens", None])
                return B.WM_OK
            self.calls.append(["wm_set_given_tokens", dict(tokens=_at(tokens.value, "int32", (n, stride)).tolist(), stride=stride,
                                                           lens=_at(lens.value, "int32", (n,)).tolist(), n=n)])
            return B.WM_OK
        self.wm_set_given_tokens = put


def given_ctx():
    c = object.__new__(B.Context)
    c.lib, c.handle = GivenLib(), ctypes.c_void_p(0xC0DE)
    c.dims = dict(n_mels=80, n_text_ctx=64, n_vocab=128)
    c.lib.blob = ("float32", (MEL.size,))
    return c


def names(ctx):
    return [c[0] for c in ctx.lib.calls]


def windows(c, n=3):
    c.lib.n_windows = n
    return B.Windows(c, ctypes.c_void_p(SET_HANDLE), np.arange(n, dtype=np.int32) + 2)


WIN = (MEL, BASE3, LEN3, SEEK3, NF3)


def test_set_given_tokens_packs_the_table():
    c = given_ctx()
    c.set_given_tokens([[5, 6, 7], [], [9]])
    assert c.lib.calls == [["wm_set_given_tokens", dict(tokens=[[5, 6, 7], [0, 0, 0], [9, 0, 0]], stride=3, lens=[3, 0, 1], n=3)]]
    assert c.lib.wm_set_given_tokens.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    c.set_given_tokens([None, np.array([4, 4], np.int64)])
    assert c.lib.calls[-1][1] == dict(tokens=[[0, 0], [4, 4]], stride=2, lens=[0, 2], n=2)
    c.set_given_tokens([[], []])                                       # a table of free rows is still a table
    assert c.lib.calls[-1][1] == dict(tokens=[[0], [0]], stride=1, lens=[0, 0], n=2)
    for drop in (None, []):
        c.set_given_tokens(drop)
        assert c.lib.calls[-1] == ["wm_set_given_tokens", None]


def test_every_wrapper_arms_right_in_front_of_its_call():
    g3 = [[7, 8], [], [9, 9, 9]]
    plain = {
        "wm_transcribe_mel": lambda c, **kw: c.transcribe_mel(*WIN, P3, 4, eot=50, **kw),
        "wm_transcribe_mel_ragged": lambda c, **kw: c.transcribe_mel(*WIN, RAGGED, 4, eot=50, sot_tail=3, budgets=[4, 3, 2], **kw),
        "wm_transcribe_windows": lambda c, **kw: c.transcribe_windows(windows(c), None, P3, 4, eot=50, **kw),
    }
    for entry, call in plain.items():
        c0, c1, c2 = given_ctx(), given_ctx(), given_ctx()
        r0, r1 = call(c0), call(c1, given=g3)
        assert "wm_set_given_tokens" not in names(c0)
        assert names(c1)[-2:] == ["wm_set_given_tokens", entry]
        assert [x for x in c1.lib.calls if x[0] != "wm_set_given_tokens"] == c0.lib.calls, entry     # nothing else moves
        assert c1.lib.calls[-2][1] == dict(tokens=[[7, 8, 0], [0, 0, 0], [9, 9, 9]], stride=3, lens=[2, 0, 3], n=3)
        assert np.array_equal(r1.tokens, r0.tokens)
        call(c2, given=g3, alternatives=2)                                 # the table goes behind the request for alternatives
        assert names(c2)[-3:] == ["wm_request_alternatives", "wm_set_given_tokens", entry]
    g6 = [[1], [2, 2], [], [3], [4, 4, 4], []]
    best = {
        "wm_transcribe_mel_best_of": lambda c, **kw: c.transcribe_mel_best_of(*WIN, P3, 4, 2, eot=50, **kw),
        "wm_transcribe_windows": lambda c, **kw: c.transcribe_windows_best_of(windows(c), None, P3, 4, 2, eot=50, **kw),
    }
    for entry, call in best.items():
        c1 = given_ctx()
        call(c1, given=g6, budgets=[1, 2, 3])
        assert names(c1)[0] == "wm_set_token_budgets" and names(c1)[-2:] == ["wm_set_given_tokens", entry]
        assert c1.lib.calls[-2][1]["lens"] == [1, 2, 0, 1, 3, 0] and c1.lib.calls[-2][1]["n"] == 6   # [B][best_of]
    c = given_ctx()
    c.transcribe_mel(*WIN, P3, 4, eot=50, best_of=2, given=g6)
    assert names(c)[-2:] == ["wm_set_given_tokens", "wm_transcribe_mel_best_of"]
    # (the stand-in has no signature for wm_transcribe and the *_aligned entries: those wrappers run in tests/test_given_gpu.py)


def test_bad_values_raise_before_any_library_call():
    assert B.given_arg(None) is None and B.given_arg(None, beam_size=2, draft=object()) is None
    tok, lens = B.given_arg([[1, 2], None, ()])
    assert tok.dtype == np.int32 and tok.tolist() == [[1, 2], [0, 0], [0, 0]] and lens.dtype == np.int32 and lens.tolist() == [2, 0, 0]
    for bad in ([], [[1.5]], [[-1]], [[1 << 31]], 7, [["a"]]):
        with pytest.raises(ValueError):
            B.given_arg(bad)
    with pytest.raises(ValueError, match="beam"):
        B.given_arg([[1]], beam_size=2)
    with pytest.raises(ValueError, match="draft"):
        B.given_arg([[1]], draft=object())
    c = given_ctx()
    for kw in (dict(beam_size=2), dict(beam_size=2, patience=1.5), dict(given=[[-3], [], []])):
        kw.setdefault("given", [[1], [2], [3]])
        for call in (lambda: c.transcribe_mel(*WIN, P3, 4, eot=50, budgets=[1, 1, 1], **kw),
                     lambda: c.transcribe_windows(windows(c), None, P3, 4, eot=50, budgets=[1, 1, 1], **kw)):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: c.transcribe_mel_raw(*WIN, P3, 4, 50, given=[[-1]], budgets=[1, 1, 1]),
                 lambda: c.transcribe_mel_best_of(*WIN, P3, 4, 2, eot=50, given=[[2.5]], budgets=[1, 1, 1])):
        with pytest.raises(ValueError):
            call()
    assert c.lib.calls == []


def test_score_given_is_one_best_of_call_where_every_window_has_k_texts():
    c = given_ctx()
    texts = [[[5, 6], [7]], [[8], [9, 10, 11]], [[12], [13]]]
    out = B.score_given(c, windows(c), None, P3, texts, 50, length_penalty=0.5)
    assert names(c) == ["wm_set_token_budgets", "wm_set_given_tokens", "wm_transcribe_windows"]
    assert c.lib.calls[0][1]["budgets"]["values"] == [3, 4, 2]             # per window: its longest text with eot
    tab = c.lib.calls[1][1]
    assert tab["n"] == 6 and tab["stride"] == 4 and tab["lens"] == [3, 2, 2, 4, 2, 2]
    assert tab["tokens"][0] == [5, 6, 50, 0] and tab["tokens"][3] == [9, 10, 11, 50]
    call = c.lib.calls[2][1]
    assert call["N"] == 2 and call["max_new"] == 4 and call["B"] == 3 and call["length_penalty"] == 0.5 and call["eot"] == 50
    assert call["opts"]["temperature"] == 0.0 and call["rows"]["values"] == [0, 1, 2]
    assert [[a.tolist() for a in r] for r in out.logprobs] == [[[-0.5] * 3, [-0.5] * 2], [[-0.5] * 2, [-0.5] * 4], [[-0.5] * 2] * 2]
    assert out.sum_logprob[1] == [-1.0, -2.0] and out.avg_logprob[1] == [-0.5, -0.5] and out.best.tolist() == [0, 1, 0]
    # without the eot: the texts as they are
    c = given_ctx()
    out = B.score_given(c, windows(c), [2, 0], P3[0], [texts[2], texts[0]], 50, append_eot=False, alternatives=2)
    assert names(c) == ["wm_set_token_budgets", "wm_request_alternatives", "wm_set_given_tokens", "wm_transcribe_windows"]
    assert c.lib.calls[2][1]["lens"] == [1, 1, 2, 1] and c.lib.calls[3][1]["rows"]["values"] == [2, 0]
    assert out.avg_logprob == [[-0.25, -0.25], [-1 / 3, -0.25]]
    assert out.alt_tokens[1][0].tolist() == [[200, 201], [210, 211]] and out.entropy[1][1].shape == (1,)


def test_score_given_repeats_the_rows_where_the_counts_differ():
    c = given_ctx()
    texts = [[[5, 6]], [[8], [9, 10, 11], [4]], [[12], [13]]]
    out = B.score_given(c, windows(c), None, RAGGED, texts, 50)
    assert names(c) == ["wm_set_token_budgets", "wm_set_given_tokens", "wm_transcribe_windows"]
    assert c.lib.calls[0][1]["budgets"]["values"] == [3, 2, 4, 2, 2, 2]
    call = c.lib.calls[2][1]
    assert call["N"] == 1 and call["B"] == 6 and call["rows"]["values"] == [0, 1, 1, 1, 2, 2]
    assert call["prompt_len"]["values"] == [3, 5, 5, 5, 4, 4]                # a prompt per row: repeated with the row
    assert out.best is None and [len(r) for r in out.logprobs] == [1, 3, 2] and out.logprobs[1][1].shape == (4,)
    for bad in ([[[5]], [[6]]], [[[5]], [], [[6]]], ):
        with pytest.raises(ValueError):
            B.score_given(given_ctx(), windows(given_ctx()), None, P3, bad, 50)
    with pytest.raises(ValueError):
        B.score_given(given_ctx(), windows(given_ctx()), None, P3, [[[]], [[1]], [[2]]], 50, append_eot=False)


# ---------------------------------------------------------------- given=None: the parent goldens
def test_without_given_the_wrappers_call_logs_are_the_parents():
    with open(BC.GOLDEN_FILE) as f:
        golden = BC.json.load(f)["cases"]
    for name in sorted(BC.CASES):
        assert BC.run_case(name) == golden[name], name


def test_without_given_transcribe_longs_call_logs_are_the_parents(tmp_path):
    with open(LC.GOLDEN_FILE) as f:
        golden = LC.json.load(f)["cases"]
    vocab = LC.make_vocab(tmp_path)
    try:
        for name, case in sorted(LC.cases(vocab).items()):
            assert LC.digest(LC.run_case(case)) == golden[name]["sha256"], name
    finally:
        vocab.close()
