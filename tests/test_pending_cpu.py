"""CPU tests of the next-call state of a transcribe call (csrc/tx_pending.h) through the debug library,
which loads without a GPU: who serves which pending item (wm_pending_refusal) for every combination of the five items with
every kind of call, against the table below -- written from the "Served / Refused" paragraphs of wm_set_sampling_rows,
wm_request_alternatives, wm_set_bias_rows and wm_set_constraint_rows in include/whisper_mi355x.h and the message texts of the
code before the items became one value -- and WmPending::take."""
import ctypes
import itertools

import numpy as np
import pytest

WM_OK, WM_ERR_STATE = 0, 3   # include/whisper_mi355x.h
BUDGETS, BIAS_ROWS, CST_ROWS, SAMP_ROWS, ALT = 1, 2, 4, 8, 16
PLAIN, MEL, RAGGED, BEST_OF, BEAM = range(5)
GREEDY, F_BEAM, WINDOWS, HYP, SPEC, MULTI, F32 = 1, 2, 4, 8, 16, 32, 64

ROWS_GREEDY = "wm_transcribe_greedy takes no sampling row map (wm_set_sampling_rows)"
ROWS_CAND = "best-of and beam-search calls take no sampling row map (wm_set_sampling_rows)"
ROWS_F32 = "a sampling row map is not supported by the all-f32 precision path"
ROWS_SPEC = "speculative decoding takes no sampling row map (wm_set_sampling_rows)"
ROWS_MULTI = "multi_transcribe_greedy takes no sampling row map (wm_set_sampling_rows)"
ALT_BEAM = "alternatives are not served by beam-search calls"
ALT_F32 = "alternatives are not supported by the all-f32 precision path"
ALT_SPEC = "alternatives are not served by speculative decoding"
ALT_MULTI = "multi_transcribe_greedy does not serve alternatives (wm_request_alternatives)"

# kind: (entry, flags, n_cand), the refusal of a pending sampling row map, the refusal of a pending request for alternatives
# (None: served).  Budgets are served by every call; the two other row maps by every call that runs with tables / an automaton
# in force -- the entries that refuse those refuse the setting, not the map -- so neither ever changes an answer.
KINDS = {
    "greedy": ((PLAIN, GREEDY, 1), ROWS_GREEDY, None),
    "plain": ((PLAIN, 0, 1), None, None),
    "mel, mel_aligned": ((MEL, 0, 1), None, None),
    "ragged, ragged aligned": ((RAGGED, 0, 1), None, None),
    "windows at one sample, windows_aligned": ((BEST_OF, WINDOWS, 1), None, None),
    "windows at best_of 3": ((BEST_OF, WINDOWS, 3), ROWS_CAND, None),
    "mel_best_of at 1": ((BEST_OF, 0, 1), ROWS_CAND, None),
    "mel_best_of at 3": ((BEST_OF, 0, 3), ROWS_CAND, None),
    "windows_best_of_aligned at 1": ((BEST_OF, WINDOWS | HYP, 1), ROWS_CAND, None),
    "mel_beam": ((BEAM, F_BEAM, 2), ROWS_CAND, ALT_BEAM),
    "windows_beam at 1": ((BEAM, F_BEAM | WINDOWS, 1), ROWS_CAND, ALT_BEAM),
    "mel_beam_aligned": ((BEAM, F_BEAM | HYP, 2), ROWS_CAND, ALT_BEAM),
    "speculative": ((MEL, SPEC, 1), ROWS_SPEC, ALT_SPEC),
    "multi": ((PLAIN, GREEDY | MULTI, 1), ROWS_MULTI, ALT_MULTI),
    "f32: mel": ((MEL, F32, 1), ROWS_F32, ALT_F32),
    "f32: greedy": ((PLAIN, GREEDY | F32, 1), ROWS_GREEDY, ALT_F32),
    "f32: windows at one sample": ((BEST_OF, WINDOWS | F32, 1), ROWS_F32, ALT_F32),
    "f32: mel_best_of": ((BEST_OF, F32, 2), ROWS_CAND, ALT_F32),
    "f32: mel_beam": ((BEAM, F_BEAM | F32, 2), ROWS_CAND, ALT_BEAM),
}


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg.binding.load_debug_library()
    u, i = ctypes.c_uint, ctypes.c_int
    lib.wmdbg_pending_refusal.argtypes = [u, i, u, i, ctypes.c_char_p, i]
    lib.wmdbg_pending_refusal.restype = i
    lib.wmdbg_pending_take.argtypes = [u, u, ctypes.c_void_p]
    lib.wmdbg_pending_take.restype = i
    return lib


def answer(lib, pending, kind):
    buf = ctypes.create_string_buffer(256)
    status = lib.wmdbg_pending_refusal(pending, kind[0], kind[1], kind[2], buf, 256)
    return status, buf.value.decode()


@pytest.mark.parametrize("name", list(KINDS))
def test_who_serves_what(lib, name):
    """the three other items change no answer; an item's answer is its column of the table; with both, the alternatives' wins"""
    kind, rows_msg, alt_msg = KINDS[name]
    refused = {0: None, SAMP_ROWS: rows_msg, ALT: alt_msg, SAMP_ROWS | ALT: alt_msg or rows_msg}
    for pending in range(32):
        msg = refused[pending & (SAMP_ROWS | ALT)]
        assert answer(lib, pending, kind) == ((WM_ERR_STATE, msg) if msg else (WM_OK, "")), (name, pending)


def test_both_pending_written_out(lib):
    """Which error wins is part of the ABI.  A transcribe call asks for its row map in front of the entry's own checks and for
    its alternatives inside validation (it masks the items); the speculative and the multi entry ask for both at once."""
    both = SAMP_ROWS | ALT
    assert answer(lib, both & SAMP_ROWS, KINDS["mel_beam"][0]) == (WM_ERR_STATE, ROWS_CAND)      # a beam call: first this ...
    assert answer(lib, both & ALT, KINDS["mel_beam"][0]) == (WM_ERR_STATE, ALT_BEAM)             # ... and past it, this
    assert answer(lib, both & SAMP_ROWS, KINDS["f32: greedy"][0]) == (WM_ERR_STATE, ROWS_GREEDY)
    assert answer(lib, both & ALT, KINDS["f32: greedy"][0]) == (WM_ERR_STATE, ALT_F32)
    assert answer(lib, both & SAMP_ROWS, KINDS["f32: mel"][0]) == (WM_ERR_STATE, ROWS_F32)
    assert answer(lib, both & ALT, KINDS["mel_best_of at 3"][0]) == (WM_OK, "")
    assert answer(lib, both, KINDS["speculative"][0]) == (WM_ERR_STATE, ALT_SPEC)
    assert answer(lib, both, KINDS["multi"][0]) == (WM_ERR_STATE, ALT_MULTI)
    assert answer(lib, both | BUDGETS, KINDS["multi"][0]) == (WM_ERR_STATE, ALT_MULTI)
    assert answer(lib, SAMP_ROWS | BUDGETS, KINDS["multi"][0]) == (WM_ERR_STATE, ROWS_MULTI)
    assert answer(lib, SAMP_ROWS, KINDS["speculative"][0]) == (WM_ERR_STATE, ROWS_SPEC)


def test_bad_arguments(lib):
    buf = ctypes.create_string_buffer(8)
    assert lib.wmdbg_pending_refusal(0, 5, 0, 1, buf, 8) == -1
    assert lib.wmdbg_pending_refusal(0, -1, 0, 1, buf, 8) == -1
    assert lib.wmdbg_pending_refusal(0, 0, 0, 1, None, 8) == -1
    assert lib.wmdbg_pending_take(0, 0, None) == -1


def test_take(lib):
    """armed, then taken, then empty; the taken value does not see a later arm"""
    out = np.full(6, -7, dtype=np.int32)
    for bits, again in itertools.product(range(32), (0, 31, BUDGETS, SAMP_ROWS | ALT)):
        assert lib.wmdbg_pending_take(bits, again, out.ctypes.data_as(ctypes.c_void_p)) == 0
        armed, taken, left, taken_later, member, budget = out.tolist()
        assert (armed, taken, left) == (bits, bits, 0), (bits, again)
        assert (taken_later, member) == (bits, again), (bits, again)
        assert budget == (1 if bits & BUDGETS else 0), (bits, again)
