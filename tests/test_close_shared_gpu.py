"""The three closes of a decode position on the SAME partials: the arg-max close (argmax_embed_x_kernel), the beam close's
list kernel (beam_topk_kernel, windows of one beam) and the speculative round's accept (spec_accept_kernel, windows of w
rows), through wmdbg_decode_close_shared (include/whisper_mi355x_debug.h).  One DE_LOGITS_X launch leaves the per-tile
partials; all three read them and must take the same row decision (csrc/dec_close.h: row_choose, row_log_norm, row_logprob,
row_no_speech) -- token and log-prob BITS, no tolerance: the claim is identity.  The inputs are the sum-rule rows of
test_decode_step_kernels_gpu.py: forced and unforced rows at a reference gap of at least 0.25 either way, a row with
timestamps only, one with text only, one with nothing admissible."""
import ctypes
import types

import numpy as np
import pytest

import test_decode_step_kernels_gpu as DS
from test_decode_step_kernels_gpu import Step, allowed_sets, bits, decide, dbg, run_step, sum_rule_inputs, world   # noqa: F401 (dbg: fixture)

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int


def run_shared(dbg, w_geom, rows, width, **kw):
    """run_step with wmdbg_decode_close_shared in the place of wmdbg_decode_close: the arg-max close's outputs as run_step
    returns them, plus r.beam_n / beam_tok / beam_lp / beam_ns and r.acc_tok / acc_lp."""
    B = len(rows)
    out = types.SimpleNamespace(beam_n=np.full(B, -7, np.int32), beam_tok=np.full(B, -7, np.int32), beam_lp=np.zeros(B, np.float32),
                                beam_ns=np.zeros(B, np.float32), acc_tok=np.full(B, -7, np.int32), acc_lp=np.zeros(B, np.float32))
    fn = dbg.lib.wmdbg_decode_close_shared
    fn.argtypes = [vp, ctypes.POINTER(Step), ip] + [vp] * 6

    def close(handle, step):
        return fn(handle, step, width, DS.P(out.beam_n), DS.P(out.beam_tok), DS.P(out.beam_lp), DS.P(out.beam_ns), DS.P(out.acc_tok),
                  DS.P(out.acc_lp))
    stand_in = types.SimpleNamespace(handle=dbg.handle, lib=types.SimpleNamespace(wmdbg_decode_close=close, wm_last_error=dbg.lib.wm_last_error))
    r = run_step(stand_in, w_geom, rows, **kw)
    for k, v in vars(out).items():
        setattr(r, k, v)
    return r


def reference_gaps(w, rows, bias, rng):
    ref = w.ref[rows] + bias.astype(np.float64)
    gaps = []
    for b in range(len(rows)):
        text, tsm = allowed_sets(w.V, (), (), 0, rng[b], 0, 0)
        gaps.append(decide(ref[b], text, tsm)[3])
    return gaps


@pytest.mark.parametrize("ts_on", [True, False], ids=["rules", "norules"])
@pytest.mark.parametrize("B,width", [(8, 1), (16, 8), (40, 8)])
@pytest.mark.parametrize("geom", ["small64", "production"])
def test_three_closes_take_one_decision(dbg, geom, B, width, ts_on):
    """Per row with something admissible: accept's token == the arg-max close's, their log-probs equal as uint32, and the beam
    list's first entry equals both.  Nothing admissible: the fallback token and -inf from the arg-max and accept closes, an
    empty beam list.  And the arg-max close behind the two others returns what wmdbg_decode_close returns for the same step."""
    w = world(geom)
    rows, bias, rng, special = sum_rule_inputs(w, B)
    gaps = reference_gaps(w, rows, bias, rng)
    # a CPU condition on the inputs (as test_sum_rule_away_from_a_tie): the device logits sit within 4e-3 of the reference
    assert all(abs(g_) >= 0.25 for g_ in gaps), gaps
    assert abs(gaps[0] - 0.5) < 1e-4 and abs(gaps[1] + 0.5) < 1e-4, gaps[:2]
    # both sides of the rule among the pool rows (rows 2 ..., the special rows aside).  B = 8 has three of them, and at the
    # production geometry sum_rule_inputs draws all three on the forced side (reference gaps +0.50, +1.02, +0.43): there the
    # two sides are rows 0 and 1 and the pool rows together, which is what the condition is for.
    pool = [gaps[b] for b in range(2 if B >= 16 else 0, B) if b not in special]
    assert any(g_ > 0 for g_ in pool) and any(g_ < 0 for g_ in pool), pool
    nothing = [b for b, rg in special.items() if rg[0] == rg[1] and rg[2] == rg[3]]
    assert len(special) == 3 and len(nothing) == 1
    kw = dict(bias=bias, fallback=w.eot, xm=dict(T=0.0))
    if ts_on:
        kw["ts"] = dict(mode=2, rng=rng, hist=np.tile([3, 0, 0, -1], (B, 1)))
    else:
        nothing = []                  # (rules off: every id is admissible text)
    r = run_shared(dbg, w, rows, width, **kw)
    plain = run_step(dbg, w, rows, **kw)
    for name in ("logits", "logprob", "nospeech", "x_next", "xb_next", "stats"):
        assert np.array_equal(bits(getattr(r, name)), bits(getattr(plain, name))), name
    assert np.array_equal(r.tok, plain.tok) and np.array_equal(r.seq, plain.seq) and r.logprob_written == plain.logprob_written
    if ts_on:
        assert np.array_equal(r.rng, plain.rng) and np.array_equal(r.hist, plain.hist)
        assert r.tok[0] >= w.ts_begin and r.tok[1] < w.ts_begin          # the forced row and the unforced row
    some = np.array([b not in nothing for b in range(B)])
    print("%s B %d w %d rules %d: tokens %s" % (geom, B, width, ts_on, r.tok.tolist()))
    assert np.array_equal(r.acc_tok[some], r.tok[some]), (r.acc_tok, r.tok)
    assert np.array_equal(bits(r.acc_lp)[some], bits(r.logprob)[some]), (r.acc_lp, r.logprob)
    assert np.all(r.beam_n[some] >= 1), r.beam_n
    assert np.array_equal(r.beam_tok[some], r.tok[some]), (r.beam_tok, r.tok)
    assert np.array_equal(bits(r.beam_lp)[some], bits(r.logprob)[some]), (r.beam_lp, r.logprob)
    assert np.all(np.isfinite(r.logprob[some]))
    for b in nothing:
        assert r.tok[b] == w.eot and r.acc_tok[b] == w.eot
        assert r.logprob[b] == -np.inf and r.acc_lp[b] == -np.inf
        assert r.beam_n[b] == 0
    assert np.all(bits(r.nospeech) == DS.SENT32) and np.all(bits(r.beam_ns) == DS.SENT32)     # pos != sot_pos: untouched


@pytest.mark.parametrize("geom", ["small64", "production"])
def test_no_speech_prob_of_the_arg_max_and_beam_closes(dbg, geom):
    """sot_pos == pos, timestamp rules off: both closes write no_speech_prob, equal as uint32 (and the tokens and log-probs of
    all three closes still agree)."""
    w = world(geom)
    B, width = 16, 8
    rows, bias, _, _ = sum_rule_inputs(w, B)
    r = run_shared(dbg, w, rows, width, bias=bias, fallback=w.eot, xm=dict(T=0.0, sot_pos=3, ns_tok=33))
    assert not np.any(bits(r.nospeech) == DS.SENT32) and np.all((r.nospeech > 0) & (r.nospeech < 1))
    assert np.array_equal(bits(r.beam_ns), bits(r.nospeech)), (r.beam_ns, r.nospeech)
    assert np.array_equal(r.acc_tok, r.tok) and np.array_equal(r.beam_tok, r.tok)
    assert np.array_equal(bits(r.acc_lp), bits(r.logprob)) and np.array_equal(bits(r.beam_lp), bits(r.logprob))
