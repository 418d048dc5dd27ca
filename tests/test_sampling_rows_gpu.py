"""GPU tests of the per-row temperature and seed (wm_set_sampling_rows) through the C ABI, on the `lively`
tiny model of test_model_gpu.py (V = 1024).  Every claim is bit-for-bit equality with a call that existed before the entry:
row b of a call under the map equals transcribe_mel on that row ALONE at its scalar (temperature, seed) -- the rows carry
explicit sample ids, so the Philox counters do not depend on the row's place -- and, for wm_transcribe on PCM (whose counter word
is the call index), row b of the same call with every row at that scalar pair."""
import ctypes

import numpy as np
import pytest

from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_sampling_rules_gpu import same
from test_transcribe_options_gpu import EOT, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
PROMPT = [10, 21, 5]
RAGGED = [[10, 21, 5], [7, 9, 10, 21, 5], [5, 5, 5, 5, 5, 5, 10, 21, 5], [4, 8, 10, 21, 5], [10, 21, 5]]
NEW = 24
R = 5
TEMPS = [0.0, 0.2, 0.0, 0.8, 1.0]
SEEDS = [3, 2 ** 33 + 5, 7, 11, 2 ** 63 + 13]
IDS = [(3 << 16) | 1, (1 << 16) | 2, 7, (2 << 16) | 9, 40]
NS = 1000
FIELDS = ("tokens", "lens", "logprobs", "no_speech_prob", "alt_tokens", "alt_logprobs", "alt_counts", "entropy", "start_frames")


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(R))
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(R, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    ctx.set_sampling_rules()
    _rules(ctx, True)
    yield w
    ctx.set_lanes(0)
    ctx.set_sampling_rules()
    ctx.set_sampling_rows([], [])
    _rules(ctx, False)


def row_equal(a, i, b, j):
    """None, or the first field in which row i of result a differs from row j of result b"""
    for f in FIELDS:
        x, y = getattr(a, f, None), getattr(b, f, None)
        if (x is None) != (y is None):
            return f + " (present in one)"
        if x is not None and not same(x[i], y[j]):
            return f
    return None


def mel_rows(w, rows):
    m = w["mel_args"]
    return (m[0], m[1][list(rows)], *m[2:])


def alone(w, b, prompts=PROMPT, aligned=False, T=None, seed=None, sid=None, **kw):
    """the call that exists today: row b alone at its scalar options"""
    ctx = w["ctx"]
    fn = ctx.transcribe_mel_aligned if aligned else ctx.transcribe_mel
    p = [prompts[b]] if isinstance(prompts[0], list) else prompts
    return fn(*mel_rows(w, [b]), p, NEW, eot=EOT, no_speech_token=NS, temperature=TEMPS[b] if T is None else T,
              seed=SEEDS[b] if seed is None else seed, sample_ids=[IDS[b] if sid is None else sid], **kw)


ROWS_KW = dict(row_temperatures=TEMPS, row_seeds=SEEDS)


@pytest.mark.parametrize("name", ["mel", "ragged", "rules", "alternatives", "windows", "aligned"])
def test_every_row_is_the_row_alone_at_its_scalar_options(world, name):
    w, ctx = world, world["ctx"]
    common = dict(eot=EOT, no_speech_token=NS, sample_ids=IDS, temperature=0.5, seed=99)   # (the call's own pair is not read)
    kw_alone, prompts, aligned = {}, PROMPT, False
    try:
        if name == "mel":
            got = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **common, **ROWS_KW)
        elif name == "ragged":
            prompts, kw_alone = RAGGED, dict(sot_tail=3)
            got = ctx.transcribe_mel(*w["mel_args"], RAGGED, NEW, sot_tail=3, **common, **ROWS_KW)
        elif name == "rules":
            ctx.set_sampling_rules(8, 0.9)
            got = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **common, **ROWS_KW)
        elif name == "alternatives":
            kw_alone = dict(alternatives=3)
            got = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, alternatives=3, **common, **ROWS_KW)
        elif name == "windows":
            with ctx.encode_windows(*w["mel_args"]) as ws:
                got = ctx.transcribe_windows(ws, None, PROMPT, NEW, **common, **ROWS_KW)
        else:
            aligned = True
            got = ctx.transcribe_mel_aligned(*w["mel_args"], PROMPT, NEW, **common, **ROWS_KW)
        for b in range(R):
            one = alone(w, b, prompts, aligned, **kw_alone)
            assert row_equal(got, b, one, 0) is None, (name, b, row_equal(got, b, one, 0))
        if name == "rules":   # a temperature-0 row is untouched by the truncation: the rules-off arg-max row
            ctx.set_sampling_rules()
            for b in (0, 2):
                assert row_equal(got, b, alone(w, b), 0) is None
        # not vacuous: the sampling rows differ from their own arg-max decode
        zero = ctx.transcribe_mel(*w["mel_args"], prompts, NEW, eot=EOT, no_speech_token=NS, sample_ids=IDS, **kw_alone)
        assert sum(not same(got.tokens[b], zero.tokens[b]) for b in (1, 3, 4)) >= 2
        assert all(same(got.tokens[b], zero.tokens[b]) for b in (0, 2))
    finally:
        ctx.set_sampling_rules()


def test_transcribe_on_pcm(world):
    """wm_transcribe: the counter word is the call index, so row b is compared with row b of the call at its scalar pair"""
    ctx, pcm = world["ctx"], world["pcm"]
    got = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, no_speech_token=NS, **ROWS_KW)
    for b in range(R):
        want = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, no_speech_token=NS, temperature=TEMPS[b], seed=SEEDS[b])
        assert row_equal(got, b, want, b) is None, b


def test_more_than_one_decode_group_and_two_lanes(world):
    """130 rows (the 5 windows over and over, every window under every (temperature, seed) pair) are cut into more than one
    decode group; the same call on two lanes; each row is its window alone under its pair"""
    w, ctx = world, world["ctx"]
    B = 130
    src = [b % R for b in range(B)]
    pair = [(b // R + b) % R for b in range(B)]
    assert B > 128 and {(s, p) for s, p in zip(src, pair)} == {(s, p) for s in range(R) for p in range(R)}
    want = {(s, p): alone(w, s, T=TEMPS[p], seed=SEEDS[p]) for s in range(R) for p in range(R)}
    kw = dict(eot=EOT, no_speech_token=NS, sample_ids=[IDS[s] for s in src], row_temperatures=[TEMPS[p] for p in pair],
              row_seeds=[SEEDS[p] for p in pair])
    try:
        for lanes in (0, 2):
            ctx.set_lanes(lanes)
            got = ctx.transcribe_mel(*mel_rows(w, src), PROMPT, NEW, **kw)
            for b in range(B):
                assert row_equal(got, b, want[(src[b], pair[b])], 0) is None, (lanes, b)
        ctx.set_lanes(2)
        small = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, eot=EOT, no_speech_token=NS, sample_ids=IDS, **ROWS_KW)
        for b in range(R):
            assert row_equal(small, b, want[(b, b)], 0) is None, b
    finally:
        ctx.set_lanes(0)


def test_a_map_of_zeros_and_the_life_of_a_map(world):
    w, ctx = world, world["ctx"]
    kw = dict(eot=EOT, no_speech_token=NS, sample_ids=IDS)
    plain = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw)
    zeros = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, row_temperatures=[0.0] * R, row_seeds=SEEDS, **kw)
    assert all(row_equal(zeros, b, plain, b) is None for b in range(R))
    # consumed: the call after it runs on its own options again
    sampled = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, temperature=0.8, seed=11, **kw)
    ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, temperature=0.8, seed=11, **kw, **ROWS_KW)
    again = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, temperature=0.8, seed=11, **kw)
    assert all(row_equal(again, b, sampled, b) is None for b in range(R)) and not same(sampled.tokens, plain.tokens)
    # n = 0 drops a pending map
    ctx.set_sampling_rows(TEMPS, SEEDS)
    ctx.set_sampling_rows([], [])
    assert all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))
    # None and None drop one as well
    ctx.set_sampling_rows(TEMPS, SEEDS)
    ctx.set_sampling_rows(None, None)
    assert all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))
    # a wrapper whose own checks raise in Python, behind the map and in front of the C call, leaves no map behind
    with pytest.raises(ValueError):
        ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, prompt_len=[3, 3], **kw, **ROWS_KW)
    assert all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))
    with pytest.raises(ValueError):
        ctx.transcribe_mel_aligned(*w["mel_args"], PROMPT, NEW, prompt_len=[3, 3], **kw, **ROWS_KW)
    assert all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))
    # a call that fails consumes it too
    ctx.set_sampling_rows(TEMPS, SEEDS)
    with pytest.raises(w["b"].WhisperError):
        ctx.transcribe_mel(*w["mel_args"], PROMPT, 10 ** 6, **kw)
    assert all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))


def status_of(w, fn):
    with pytest.raises(w["b"].WhisperError) as e:
        fn()
    return e.value.status


def test_errors(world):
    w, ctx = world, world["ctx"]
    kw = dict(eot=EOT, no_speech_token=NS, sample_ids=IDS)
    plain = ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw)

    def runs_plain():   # no map is left behind: the next call is the plain one
        return all(row_equal(ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw), b, plain, b) is None for b in range(R))
    # the wrong n
    ctx.set_sampling_rows(TEMPS[:4], SEEDS[:4])
    assert status_of(w, lambda: ctx.transcribe_mel(*w["mel_args"], PROMPT, NEW, **kw)) == WM_ERR_INVALID and runs_plain()
    # bad temperatures: refused at set time, and a map that was pending is dropped
    for bad in (-0.5, float("nan"), float("inf"), 1e-42):
        ctx.set_sampling_rows(TEMPS, SEEDS)
        assert status_of(w, lambda: ctx.set_sampling_rows([0.0, bad, 0.0, 0.8, 1.0], SEEDS)) == WM_ERR_INVALID, bad
        assert runs_plain(), bad
    fn = ctx.lib.wm_set_sampling_rows
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    t = np.array(TEMPS, np.float32)
    assert fn(ctx.handle, t.ctypes.data_as(ctypes.c_void_p), None, R) == WM_ERR_INVALID
    assert fn(ctx.handle, None, None, -1) == WM_ERR_INVALID and runs_plain()
    # the refused entries: WM_ERR_STATE, and no map behind
    refused = {
        "greedy": lambda: ctx.transcribe_greedy(w["pcm"], PROMPT, NEW, eot=EOT),
        "best_of": lambda: ctx.transcribe_mel_best_of(*w["mel_args"], PROMPT, NEW, 2, eot=EOT, temperature=0.8),
        "beam": lambda: ctx.transcribe_mel_beam(*w["mel_args"], PROMPT, NEW, 2, eot=EOT),
        "best_of_aligned": lambda: ctx.transcribe_mel_best_of_aligned(*w["mel_args"], PROMPT, NEW, 2, eot=EOT, temperature=0.8),
        "beam_aligned": lambda: ctx.transcribe_mel_beam_aligned(*w["mel_args"], PROMPT, NEW, 2, eot=EOT),
    }
    with ctx.encode_windows(*w["mel_args"]) as ws:
        refused["windows_best_of"] = lambda: ctx.transcribe_windows_best_of(ws, None, PROMPT, NEW, 2, eot=EOT, temperature=0.8)
        refused["windows_beam"] = lambda: ctx.transcribe_windows_beam(ws, None, PROMPT, NEW, 2, eot=EOT)
        draft = ctx.clone()
        try:
            refused["speculative"] = lambda: ctx.transcribe_mel_speculative(draft, *w["mel_args"], PROMPT, NEW, 3, eot=EOT)
            for name, call in refused.items():
                ctx.set_sampling_rows(TEMPS, SEEDS)
                assert status_of(w, call) == WM_ERR_STATE, name
                assert runs_plain(), name
        finally:
            draft.close()


def test_the_multi_device_entry_refuses_a_map(world, pkg):
    """wm_multi_transcribe_greedy on a device context with a pending map: WM_ERR_STATE, and the map is consumed"""
    from oracle import whisper_ref as R_
    multi = pkg.binding.MultiContext(dict(R_.TINY_DIMS), devices=[0])
    try:
        multi.init_synthetic(11)
        pcm, prompt = world["pcm"], [10, 21, 5, 7]
        t0, l0 = multi.transcribe_greedy(pcm, prompt, 6)
        multi.device_ctx(0).set_sampling_rows(TEMPS, SEEDS)
        assert status_of(world, lambda: multi.transcribe_greedy(pcm, prompt, 6)) == WM_ERR_STATE
        t1, l1 = multi.transcribe_greedy(pcm, prompt, 6)          # consumed: the next call is the plain one
        assert same(t1, t0) and same(l1, l0)
        # with a request for alternatives pending too, the entry answers for that one and has consumed both
        multi.device_ctx(0).set_sampling_rows(TEMPS, SEEDS)
        multi.device_ctx(0).request_alternatives(2, R, 6)
        with pytest.raises(pkg.binding.WhisperError) as e:
            multi.transcribe_greedy(pcm, prompt, 6)
        assert e.value.status == WM_ERR_STATE and "does not serve alternatives" in str(e.value)
        t2, l2 = multi.transcribe_greedy(pcm, prompt, 6)
        assert same(t2, t0) and same(l2, l0)
    finally:
        multi.close()


def test_the_all_f32_path_refuses_a_map(world, pkg):
    w = world
    c = pkg.binding.Context(w["dims"], debug=True)
    try:
        c.load_state_dict(w["sd_np"])
        c.finalize()
        c.set_precision(True)
        c.set_sampling_rows(TEMPS, SEEDS)
        assert status_of(w, lambda: c.transcribe_mel(*w["mel_args"], PROMPT, NEW, eot=EOT, sample_ids=IDS)) == WM_ERR_STATE
        c.transcribe_mel(*w["mel_args"], PROMPT, 4, eot=EOT, sample_ids=IDS)   # no map behind: the plain call runs
    finally:
        c.close()
