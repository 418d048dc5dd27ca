"""GPU test of the next-call state's lifecycle (csrc/tx_pending.h): whatever wm_set_token_budgets,
wm_set_bias_rows, wm_set_constraint_rows, wm_set_sampling_rows and wm_request_alternatives armed is consumed by the NEXT
transcribe call, also by one that fails at its earliest argument check.  For every entry -- greedy, plain, mel, ragged,
windows, the two aligned, best-of, beam, speculative -- on the `lively` tiny model with B = 2 and max_new = 4: arm, make the
entry fail on all-null arguments (an argument error answered on the host: nothing is dereferenced, nothing is launched), then
make a valid plain call of the same B and look for a trace of the armed state.

Three rounds per entry, because tables in force change what the plain call is and a pending sampling row map is judged in front
of an entry's own checks:
  all five, tables and an automaton in force: the plain call WITHOUT a row map answers WM_ERR_STATE ("... no row map") exactly
    when the failed call consumed the bias row map;
  the other four, an automaton in force: the plain call's lengths are not clamped by the budget, the sentinel-filled
    alternatives buffers are untouched, its tokens are the unarmed call's (rows start in state 0, no row samples);
  those without the sampling row map: every entry fails at its own first argument check (WM_ERR_INVALID), the same plain call.
FAILS is what the commit before the pending state became one value answered, entry by entry; every entry consumed there."""
import ctypes

import numpy as np
import pytest

from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
B, NEW = 2, 4
PROMPT = [10, 21, 5]
SENTINEL = -77
ENTRIES = {   # the entry point of each name
    "greedy": "wm_transcribe_greedy", "plain": "wm_transcribe", "mel": "wm_transcribe_mel", "ragged": "wm_transcribe_mel_ragged",
    "windows": "wm_transcribe_windows", "mel_aligned": "wm_transcribe_mel_aligned",
    "windows_aligned": "wm_transcribe_windows_aligned", "best_of": "wm_transcribe_mel_best_of", "beam": "wm_transcribe_mel_beam",
    "speculative": "wm_transcribe_mel_speculative",
}
# The status of the all-null call with everything armed.  A pending sampling row map is judged in front of the entry's own
# checks: the entries that refuse it answer WM_ERR_STATE; the others reach their first argument check.  (wm_transcribe_windows
# is the best-of entry of a window set and serves the map at best_of == 1 alone: the all-null call's best_of is 0.)
FAILS = {"greedy": WM_ERR_STATE, "plain": WM_ERR_INVALID, "mel": WM_ERR_INVALID, "ragged": WM_ERR_INVALID, "windows": WM_ERR_STATE,
         "mel_aligned": WM_ERR_INVALID, "windows_aligned": WM_ERR_INVALID, "best_of": WM_ERR_STATE, "beam": WM_ERR_STATE,
         "speculative": WM_ERR_INVALID}


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    b = pkg.binding
    mel = ctx.logmel(tones(B), out_dtype=np.float32)
    w = dict(ctx=ctx, b=b, mel_args=(mel.reshape(-1), np.arange(B, dtype=np.int64) * 80 * 3000, 3000, 0, 3000))
    # two disjoint one-phrase grammars in one automaton: a row started in the second one cannot decode what state 0 allows
    w["automaton"], w["starts"] = b.constraint_join([b.constraint_from_choices([[3, 4, 5, 6]]), b.constraint_from_choices([[7, 8, 9, 11]])])
    ctx.set_constraint(w["automaton"], eot=dims["n_vocab"] - 1)
    w["unarmed"] = plain(w)
    yield w
    ctx.set_sequence_bias_tables([])
    ctx.set_constraint(None)
    ctx.set_token_budgets([])
    ctx.set_sampling_rows([], [])
    ctx.request_alternatives(None, 0, 0)


def plain(w):
    return w["ctx"].transcribe_mel(*w["mel_args"], PROMPT, NEW)


def arm(w, tables, rows=True):
    """everything a setter can arm for the next call; -> the Alternatives whose sentinel-filled arrays that call would fill"""
    ctx = w["ctx"]
    ctx.set_token_budgets([1] * B)
    if tables:
        ctx.set_bias_rows([0] * B)
    ctx.set_constraint_rows([w["starts"][1]] * B)
    if rows:
        ctx.set_sampling_rows([1.0] * B, [5, 6])
    alt = ctx.request_alternatives(2, B, NEW)
    for a in (alt.tokens, alt.logprobs, alt.counts, alt.entropy):
        a.fill(SENTINEL)
    return alt


def untouched(alt):
    return all((a == SENTINEL).all() for a in (alt.tokens, alt.logprobs, alt.counts, alt.entropy))


def all_null(ctx, name):
    """the entry on null pointers and zeros: its earliest argument check answers; -> the status"""
    fn = getattr(ctx.lib, ENTRIES[name])
    zero = {ctypes.c_void_p: None, ctypes.c_int: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0}
    return fn(ctx.handle, *[zero[t] for t in fn.argtypes[1:]])


def test_the_armed_state_is_live(world):
    """not vacuous: the valid plain call right behind the setters shows every one of them"""
    w = world
    alt = arm(w, tables=False)
    r = plain(w)
    assert (r.lens == 1).all() and not untouched(alt)
    assert not np.array_equal(r.tokens[:, 0], w["unarmed"].tokens[:, 0])   # the other grammar, and sampled
    assert np.array_equal(plain(w).tokens, w["unarmed"].tokens) and (w["unarmed"].lens == NEW).all()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_failed_call_consumes_everything(world, name):
    w, ctx = world, world["ctx"]
    # all five, tables in force
    ctx.set_sequence_bias_tables([{(5,): 1.0}])
    try:
        alt = arm(w, tables=True)
        status = all_null(ctx, name)
        print(name, "all five armed: status", status)
        assert status == FAILS[name]
        with pytest.raises(w["b"].WhisperError) as e:
            plain(w)
        assert e.value.status == WM_ERR_STATE and "the call has no row map" in str(e.value)   # the bias row map is gone
        assert untouched(alt)
    finally:
        ctx.set_sequence_bias_tables([])
    # the other four; then without the sampling row map, so that every entry reaches its own first argument check
    for rows in (True, False):
        alt = arm(w, tables=False, rows=rows)
        status = all_null(ctx, name)
        print(name, "four armed:" if rows else "three armed:", "status", status)
        assert status == (FAILS[name] if rows else WM_ERR_INVALID)
        r = plain(w)
        assert (r.lens == NEW).all(), "clamped by the budget of the failed call"
        assert untouched(alt), "the failed call's request for alternatives was served"
        assert np.array_equal(r.tokens, w["unarmed"].tokens), "start states or sampling rows of the failed call"
