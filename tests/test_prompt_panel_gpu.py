"""wm_set_prompt_panel end to end: every transcribe entry that takes part at panel widths 2, 3 and 8 against the SAME call on
the same context at width 1, on the raw bits of every output (tokens, lengths, token log-probs, no_speech_prob, start frames)
-- the width is a launch policy, not a numerics switch --; the entries that ignore the width; what the prefill enqueued
(wmdbg_last_prompt_prefill against the plan); the setter's checks and its inheritance; transcribe_long(prompt_panel=...).
Model: tiny.en geometry, device-generated synthetic weights with the `lively` matrix gain."""
import ctypes

import numpy as np
import pytest

from test_longform_gpu import SOT_PREV, _kw, _long_recs, _strip, prod  # noqa: F401  (prod: fixture)
from test_model_gpu import tones

pytestmark = pytest.mark.gpu

EOT, SOT, NS, TSB = 50256, 50257, 50361, 50363   # tiny.en
TAIL = [SOT, 50300, 50358]                        # the 3-token sot tail
HEADS = [(1, 0), (1, 3), (3, 2), (3, 5)]
NEW = 5
WIDTHS = (2, 3, 8)
IP = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def tiny(pkg):
    ctx = pkg.binding.Context(dict(pkg.binding.MODEL_DIMS["tiny.en"]), debug=True)
    ctx.init_synthetic(23, matrix_gain=4.0)
    ctx.finalize()
    ctx.set_alignment_heads(HEADS)
    lib = ctx.lib
    lib.wmdbg_prompt_panel_plan.argtypes = [ctypes.c_int] * 5 + [IP]
    lib.wmdbg_prompt_panel_plan.restype = ctypes.c_int
    lib.wmdbg_last_prompt_prefill.argtypes = [ctypes.c_void_p, IP]
    lib.wmdbg_last_prompt_prefill.restype = ctypes.c_int
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def mel3(tiny):
    return tiny.logmel(tones(3), out_dtype=np.float32)   # [3][80][3000]


def _base(n):
    return (np.arange(n, dtype=np.int64) % 3) * (80 * 3000)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            assert x is None and y is None, (what, i)
        else:
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i)


def _fields(r):
    """the outputs of a call as a list of arrays: a raw tuple, or a result object's fields (start frames when it has them)"""
    if isinstance(r, tuple):
        return list(r)
    out = [r.tokens, r.lens, r.logprobs, r.no_speech_prob]
    if getattr(r, "start_frames", None) is not None:
        out.append(r.start_frames)
    for name in ("best", "n_hyp", "sum_logprob"):
        if getattr(r, name, None) is not None:
            out.append(getattr(r, name))
    return out


def _last(ctx, handle=None):
    out = np.full(3, -1, dtype=np.int32)
    assert ctx.lib.wmdbg_last_prompt_prefill(ctx.handle if handle is None else handle, out.ctypes.data_as(IP)) == 0
    return out.tolist()


def _plan(ctx, G, width, P, sot_pos=-1, acap_base=-1):
    out = np.zeros(5, dtype=np.int32)
    assert ctx.lib.wmdbg_prompt_panel_plan(G, width, P, sot_pos, acap_base, out.ctypes.data_as(IP)) == 0
    P0, C, w, slices, steps = out.tolist()
    return [P0, slices, slices * steps] if w else [0, 0, 0]


def _at_widths(ctx, fn, what, widths=WIDTHS, expect=None):
    """fn() at width 1, then at every width: the same bits; expect(width) = what the prefill must have enqueued"""
    want = _fields(fn())
    if expect is not None:
        assert _last(ctx) == [0, 0, 0], what
    try:
        for w in widths:
            ctx.set_prompt_panel(w)
            _same(_fields(fn()), want, "%s, width %d" % (what, w))
            if expect is not None:
                assert _last(ctx) == expect(w), (what, w)
    finally:
        ctx.set_prompt_panel(1)
    return want


def _text(rng, n):
    return [int(t) for t in rng.integers(0, EOT, size=n)]


def _rules(ctx, on=True):
    if on:
        ctx.set_suppress([SOT, SOT_PREV, NS, 220], [EOT])
        ctx.set_timestamp_rules(True, TSB, EOT, 50)
    else:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])


def _ragged_prompts(n, seed, prev=(0, 1, 17, 8, 3)):
    rng = np.random.default_rng(seed)
    return [_text(rng, prev[b % len(prev)]) + TAIL for b in range(n)]


def _ragged(ctx, b, mel, prompts, ns, T=0.0, new=NEW, eot=-1, ids=None, budgets=None, seed=77):
    opts = b.wm_decode_opts(T, seed, NS if ns else -1, 0)
    return ctx.transcribe_mel_raw(mel, _base(len(prompts)), 3000, 0, 3000, prompts, new, eot, opts, sample_ids=ids, logprobs=True,
                                  no_speech=ns, budgets=budgets, sot_tail=3)


# ---------------------------------------------------------------- 1. uniform prompts
@pytest.mark.parametrize("ns", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_uniform_prompts_are_bit_identical_at_every_width(tiny, pkg, mel3, B, ns):
    b = pkg.binding
    rng = np.random.default_rng(10 * B + ns)
    ran = 0
    for prev in (0, 1, 2, 7, 8, 9, 17):
        prompts = np.array([_text(rng, prev) + TAIL for _ in range(B)], dtype=np.int32)
        P, sot = prev + 3, prev
        opts = b.wm_decode_opts(0.0, 0, NS if ns else -1, sot)

        def run():
            return tiny.transcribe_mel_raw(mel3, _base(B), 3000, 0, 3000, prompts, NEW, -1, opts, logprobs=True, no_speech=ns)

        want = _at_widths(tiny, run, "B %d, previous text %d" % (B, prev),
                          expect=lambda w: _plan(tiny, B, w, P, sot if ns else -1))
        assert np.isfinite(want[2]).all() and (not ns or np.isfinite(want[3]).all())
        P0 = sot if ns else P - 1
        ran += P0 >= 2
        assert (_plan(tiny, B, 8, P, sot if ns else -1) != [0, 0, 0]) == (P0 >= 2)
    assert ran >= 4
    # the issue's example: P0 = 17, w = 8, B = 3 is 3 panel steps in 1 slice
    assert _plan(tiny, 3, 8, 20, 17) == [17, 1, 3]


# ---------------------------------------------------------------- 2. ragged prompts
@pytest.mark.parametrize("ns", [False, True])
@pytest.mark.parametrize("Bn,prev", [(5, (0, 1, 17, 8, 3)), (17, (0, 1, 17, 8, 3)), (48, (0, 1, 16, 8, 3))])
def test_ragged_prompts_are_bit_identical_at_every_width(tiny, pkg, mel3, Bn, prev, ns):
    """rows with off = 0 (the longest), rows that start in the middle of a panel, rows idle for whole panels; 17 rows run as one
    narrowed panel, 48 rows (P0 = 16 with no_speech_prob) as three slices"""
    b = pkg.binding
    prompts = _ragged_prompts(Bn, 3 * Bn, prev)
    P = max(prev) + 3
    sot = P - 3 if ns else -1
    tiny.set_lanes(1)
    try:
        _at_widths(tiny, lambda: _ragged(tiny, b, mel3, prompts, ns), "%d ragged rows" % Bn,
                   expect=lambda w: _plan(tiny, Bn, w, P, sot))
    finally:
        tiny.set_lanes(0)
    if Bn == 17:
        assert _plan(tiny, 17, 8, P, sot)[1] == 1
    if Bn == 48 and ns:
        assert _plan(tiny, 48, 8, P, sot) == [16, 3, 6]


def test_ragged_prompts_in_two_groups_and_under_explicit_lanes(tiny, pkg, mel3):
    b = pkg.binding
    prompts = _ragged_prompts(130, 5)      # 130 rows: two decode groups of 65
    _at_widths(tiny, lambda: _ragged(tiny, b, mel3, prompts, True, new=4), "130 rows", widths=(8,))
    prompts = _ragged_prompts(24, 6)
    want = _fields(_ragged(tiny, b, mel3, prompts, True))
    tiny.set_lanes(2)
    try:
        got = _at_widths(tiny, lambda: _ragged(tiny, b, mel3, prompts, True), "set_lanes(2)", widths=(3, 8))
    finally:
        tiny.set_lanes(0)
    _same(got, want, "set_lanes(2) against the default lanes")


def test_a_prompt_that_fills_the_context(tiny, pkg, mel3):
    b = pkg.binding
    n_ctx = tiny.dims["n_text_ctx"]
    rng = np.random.default_rng(4)
    prompts = np.array([_text(rng, n_ctx - NEW - 3) + TAIL for _ in range(2)], dtype=np.int32)
    assert prompts.shape[1] + NEW == n_ctx
    opts = b.wm_decode_opts(0.0, 0, NS, prompts.shape[1] - 3)
    _at_widths(tiny, lambda: tiny.transcribe_mel_raw(mel3, _base(2), 3000, 0, 3000, prompts, NEW, -1, opts, no_speech=True),
               "n_prompt + max_new == n_text_ctx", widths=(3, 8), expect=lambda w: _plan(tiny, 2, w, prompts.shape[1], prompts.shape[1] - 3))
    # ... and ragged: the longest row fills it, the others start late
    ragged = [_text(rng, n) + TAIL for n in (n_ctx - NEW - 3, 0, 200)]
    _at_widths(tiny, lambda: _ragged(tiny, b, mel3, ragged, False), "ragged, the longest fills the context", widths=(8,))


# ---------------------------------------------------------------- 3. every rule family
@pytest.mark.parametrize("family", ["suppress + timestamp rules", "repetition rules + sequence bias", "budgets", "early stop on eot",
                                    "temperature 0.7"])
def test_every_rule_family_on(tiny, pkg, mel3, family):
    b = pkg.binding
    prompts = _ragged_prompts(5, 21)
    kw = {}
    if family == "repetition rules + sequence bias":   # text ids alone, so that any generated token may end a biased sequence
        tiny.set_suppress(list(range(EOT, tiny.dims["n_vocab"])), [])
    else:
        _rules(tiny)
    try:
        free = _fields(_ragged(tiny, b, mel3, prompts, True))   # what the rows generate without the family's own setting
        if family == "repetition rules + sequence bias":
            assert free[0].max() < EOT
            tiny.set_repetition_rules(1.3, 2, EOT)
            tiny.set_sequence_bias({(int(free[0][0, 0]),): float("-inf"), (int(free[0][1, 0]), int(free[0][1, 1])): -4.0,
                                    (int(free[0][2, 1]), 17): 2.5}, boost=[(int(free[0][2, 1]), 17)], eot=EOT)
        elif family == "budgets":
            kw = dict(budgets=[1, 2, NEW, 1, 2])
        elif family == "early stop on eot":
            kw = dict(eot=int(free[0][1, 1]))    # row 1 stops at its second token
        elif family == "temperature 0.7":
            kw = dict(T=0.7, seed=1234, ids=np.array([(3 << 16) | 17, 5, 1 << 16, 0xFFFF, 9], dtype=np.uint32))
        want = _at_widths(tiny, lambda: _ragged(tiny, b, mel3, prompts, True, **kw), family,
                          expect=lambda w: _plan(tiny, 5, w, 20, 17))
        if family == "repetition rules + sequence bias":
            assert want[0][0, 0] != free[0][0, 0]          # the bad word is gone: the table was in force
        elif family == "budgets":
            assert want[1].tolist() == [1, 2, NEW, 1, 2]
        elif family == "early stop on eot":
            assert want[1][1] <= 2 < NEW                   # row 1 stopped early
        elif family == "temperature 0.7":
            assert np.isfinite(want[2]).all()
    finally:
        tiny.set_sequence_bias(None)
        tiny.set_repetition_rules(1.0, 0, EOT)
        _rules(tiny, False)


# ---------------------------------------------------------------- 4. every entry that takes part
def test_every_participating_entry(tiny, pkg, mel3):
    rng = np.random.default_rng(8)
    pcm = tones(2)
    prompt = _text(rng, 9) + TAIL            # P = 12, sot_index 9
    expect_ns = lambda w: _plan(tiny, 2, w, 12, 9)          # noqa: E731
    expect_last = lambda w: _plan(tiny, 2, w, 12, -1)       # noqa: E731
    _rules(tiny)
    try:
        _at_widths(tiny, lambda: tiny.transcribe_greedy(pcm, prompt, NEW, EOT), "transcribe_greedy", expect=expect_last)
        _at_widths(tiny, lambda: tiny.transcribe(pcm, prompt, NEW, EOT, no_speech_token=NS, sot_index=9), "transcribe", expect=expect_ns)
        _at_widths(tiny, lambda: tiny.transcribe(pcm, prompt, NEW, EOT, temperature=0.7, seed=3), "transcribe, sampled", expect=expect_last)
        win = (mel3, _base(2), 3000, 0, 3000)
        _at_widths(tiny, lambda: tiny.transcribe_mel(*win, [prompt, prompt], NEW, EOT, no_speech_token=NS, sot_index=9), "transcribe_mel",
                   expect=expect_ns)
        ragged = [prompt, prompt[4:]]
        _at_widths(tiny, lambda: tiny.transcribe_mel(*win, ragged, NEW, EOT, no_speech_token=NS, sot_tail=3), "transcribe_mel, ragged",
                   expect=expect_ns)
        # the aligned entries: P0 is capped at the first captured position, <|startoftranscript|>, with or without no_speech_prob
        aligned = lambda w: _plan(tiny, 2, w, 12, -1, 9)    # noqa: E731
        for nst in (-1, NS):
            r = _at_widths(tiny, lambda: tiny.transcribe_mel_aligned(*win, [prompt, prompt], NEW, EOT, no_speech_token=nst, sot_index=9),
                           "transcribe_mel_aligned", expect=aligned)
            assert (r[4][:, 0] >= 0).all()       # start frames came out
        _at_widths(tiny, lambda: tiny.transcribe_mel_aligned(*win, ragged, NEW, EOT, no_speech_token=NS, sot_tail=3),
                   "transcribe_mel_aligned, ragged", expect=aligned)
        with tiny.encode_windows(*win) as ws:
            _at_widths(tiny, lambda: tiny.transcribe_windows(ws, [1, 0], [prompt, prompt], NEW, EOT, no_speech_token=NS, sot_index=9),
                       "transcribe_windows", expect=expect_ns)
            _at_widths(tiny, lambda: tiny.transcribe_windows(ws, None, ragged, NEW, EOT, sot_tail=3), "transcribe_windows, ragged",
                       expect=expect_last)
            _at_widths(tiny, lambda: tiny.transcribe_windows_aligned(ws, [1, 0], ragged, NEW, EOT, no_speech_token=NS, sot_tail=3),
                       "transcribe_windows_aligned", expect=aligned)
    finally:
        _rules(tiny, False)
    assert _plan(tiny, 2, 8, 12, 9) == [9, 1, 2] and _plan(tiny, 2, 8, 12, -1) == [11, 1, 2]


# ---------------------------------------------------------------- 5. entries that ignore the width
def test_best_of_beam_and_speculative_calls_ignore_the_width(tiny, pkg, mel3):
    rng = np.random.default_rng(9)
    prompt = _text(rng, 17) + TAIL
    win = (mel3, _base(2), 3000, 0, 3000)
    none = lambda w: [0, 0, 0]   # noqa: E731
    _rules(tiny)
    draft = tiny.clone()
    try:
        draft.set_suppress([SOT, SOT_PREV, NS, 220], [EOT])
        draft.set_timestamp_rules(True, TSB, EOT, 50)
        _at_widths(tiny, lambda: tiny.transcribe_mel_best_of(*win, [prompt, prompt], NEW, 2, EOT, temperature=0.7, seed=5,
                                                             no_speech_token=NS, sot_index=17), "best-of", widths=(8,), expect=none)
        _at_widths(tiny, lambda: tiny.transcribe_mel_beam(*win, [prompt, prompt], NEW, 2, EOT, no_speech_token=NS, sot_index=17),
                   "beam search", widths=(8,), expect=none)
        plain = _fields(tiny.transcribe_mel(*win, [prompt, prompt], NEW, EOT, no_speech_token=NS, sot_index=17))[:4]

        def spec():
            r = tiny.transcribe_mel_speculative(draft, *win, [prompt, prompt], NEW, 3, EOT, no_speech_token=NS, sot_index=17)
            return (r.tokens, r.lens, r.logprobs, r.no_speech_prob)

        _same(_at_widths(tiny, spec, "speculative", widths=(8,), expect=none), plain, "speculative against the plain call")
    finally:
        draft.close()
        _rules(tiny, False)


# ---------------------------------------------------------------- 6. the caches, clones, the setter
def test_results_do_not_depend_on_what_the_caches_held(tiny, pkg, mel3):
    """The ragged batch twice at width 8; in between a uniform call whose prompts are the same rows padded on the LEFT with other
    tokens, so that the self-K/V rows in front of every offset and the token buffer hold other contents."""
    b = pkg.binding
    prev = (0, 1, 17, 8, 3)
    prompts = _ragged_prompts(5, 31, prev)
    rng = np.random.default_rng(99)
    want = _fields(_ragged(tiny, b, mel3, prompts, True))
    tiny.set_prompt_panel(8)
    try:
        first = _fields(_ragged(tiny, b, mel3, prompts, True))
        padded = np.array([_text(rng, 20 - len(p)) + p for p in prompts], dtype=np.int32)
        tiny.transcribe_mel_raw(mel3, _base(5), 3000, 0, 3000, padded, NEW, -1, b.wm_decode_opts(0.0, 1, NS, 17), no_speech=True)
        second = _fields(_ragged(tiny, b, mel3, prompts, True))
    finally:
        tiny.set_prompt_panel(1)
    _same(first, want, "width 8")
    _same(second, want, "width 8 over other cache contents")


def test_a_clone_inherits_the_width_and_the_setter_checks_it(tiny, pkg, mel3):
    b = pkg.binding
    prompts = _ragged_prompts(3, 41)
    want = _fields(_ragged(tiny, b, mel3, prompts, True))
    tiny.set_prompt_panel(8)
    try:
        c2 = tiny.clone()
        try:
            _same(_fields(_ragged(c2, b, mel3, prompts, True)), want, "a clone made at width 8")
            assert _last(tiny, c2.handle) == _plan(tiny, 3, 8, 20, 17) == [17, 1, 3]
        finally:
            c2.close()
    finally:
        tiny.set_prompt_panel(1)
    for bad in (0, 9):
        with pytest.raises(b.WhisperError) as e:
            tiny.set_prompt_panel(bad)
        assert e.value.status == 1 and "set_prompt_panel: width %d outside [1, 8]" % bad in str(e.value)
    _same(_fields(_ragged(tiny, b, mel3, prompts, True)), want, "after the refused widths")   # ... which left width 1 in force
    assert _last(tiny) == [0, 0, 0]


# ---------------------------------------------------------------- 7. long form
def test_conditioned_long_form_with_prompt_panels(prod):
    """the two shortest recordings with speech through the conditioned path: every window's prompt carries the previous text"""
    recs = _long_recs()[:2]
    rng = np.random.default_rng(21)
    seeds = [[int(t) for t in rng.integers(0, 50000, size=n)] for n in (5, 2)]
    kw = dict(recording_ids=[7, 300], condition_on_previous_text=True, sot_prev=SOT_PREV, initial_prompt_tokens=seeds,
              **_kw(logprob_threshold=None, compression_ratio_threshold=None))
    want = prod.transcribe_long(recs, **kw)
    assert max(w["prompt_len"] for o in want for w in o["windows"]) >= 6
    try:
        got = prod.transcribe_long(recs, prompt_panel=8, **kw)
    finally:
        prod.set_prompt_panel(1)
    assert [_strip(o) for o in got] == [_strip(o) for o in want]
    assert [[w["prompt"] for w in o["windows"]] for o in got] == [[w["prompt"] for w in o["windows"]] for o in want]
    assert [_strip(o) for o in prod.transcribe_long(recs, prompt_panel=None, **kw)] == [_strip(o) for o in want]
