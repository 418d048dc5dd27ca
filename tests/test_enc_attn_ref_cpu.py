"""tests/enc_attn_ref.py held to its conditions, on the CPU: the restatement equals a triple loop; an emulation of the kernel's
order of operations stays inside the derived bound on every input the GPU tests use, and inside the exact probes' gate; each
value-only mistake the bound is meant to catch exceeds it on those inputs; the "peaked" input really takes late moves of the
softmax reference.

Measured here (largest error / bound over all spread cases): the emulation 0.79 with the f32 row sum, 0.61 against the SUM_MFMA
bound with the row sum of the rounded P; the f32 terms are at most 0.11 of the bound.  Moves after the first tile on the peaked
input: 390 at (B, H, S) = (1, 1, 1500), 2172 at (3, 2, 1500), 21 at (3, 2, 193), none on the normal input.  Mutants, smallest
largest-error / bound over the cases that can show them: last key dropped 8.2 (S = 1500; >= 21 below), one key doubled 11.0,
alpha = 2^(-delta / 2) 285, alpha on half the accumulators 2155, per-lane move with a stale C operand 32 (193) .. 1838 (1500).

The row sum taken from the rounded P is NOT over the bound of the f32 row sum on these inputs (largest 0.75), and cannot be
expected to be: its error is sum_j (P_j - p_j)(v_j - ref) / l, at most u (A + |ref|) before the output rounding, the same first-
order size as the honest kernel's u A; and it is what the kernel's own SUM_MFMA variant computes.  It is held to that variant's
bound instead, u (A + 2 |ref|) + f32 terms (test_row_sum_of_rounded_p_has_its_own_bound)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_attn_ref as E   # noqa: E402

_CACHE = {}


def spread(case):
    """(q, k, v, restatement) of a spread case, computed once"""
    if case not in _CACHE:
        B, H, S, kind = case
        q, k, v = E.spread_inputs(B, H, S, kind)
        _CACHE[case] = (q, k, v, E.restate(q, k, v, H))
    return _CACHE[case]


def worst(out, r, variant=0):
    return float((np.abs(out.astype(np.float64) - r.ref) / r.bound[variant]).max())


def case_id(c):
    return "B%d-H%d-S%d-%s" % c


CASES = E.spread_cases()
MUTANT_CASES = [c for c in CASES if c[:2] != (1, 1)]      # the (1, 1) shapes repeat the (3, 2) ones for the emulation


def test_constants_and_rounding():
    assert abs(float(E.QSCALE) - 0.125 * np.log2(np.e)) <= 2.0 ** -24 * 0.19
    x = np.array([1.0, 1.00390625, 1.01171875, 256.0, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)    # two ties: to even
    assert np.array_equal(E.bf16(x), np.array([1.0, 1.0, 1.015625, 256.0, 1.0078125], np.float32))
    assert E.bf16_ulp(1.0) == 2.0 ** -7 and E.bf16_ulp(0.75) == 2.0 ** -8 and E.bf16_ulp(0.0) == 0.0


def test_restatement_equals_a_triple_loop():
    B, H, S = 2, 2, 5
    q, k, v = E.spread_inputs(B, H, S, "peaked")
    r = E.restate(q, k, v, H)
    ref, A = E.triple_loop(q, k, v, H)
    assert np.abs(r.ref - ref).max() <= 1e-12 and np.abs(r.A - A).max() <= 1e-12
    assert (r.bound[0] > E.U * (r.A + np.abs(r.ref))).all() and (r.bound[1] >= r.bound[0]).all()
    # the heads and chunks are told apart: a transposed (b, h) index gives another answer
    r2 = E.restate(q[::-1], k[::-1], v[::-1], H)
    assert np.abs(r2.ref[::-1] - ref).max() <= 1e-12 and np.abs(r2.ref - ref).max() > 1e-3


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_emulation_stays_inside_the_bound(case):
    B, H, S, kind = case
    q, k, v, r = spread(case)
    for variant in (0, 1):
        out, moves = E.emulate(q, k, v, H, sum_rounded=bool(variant))
        w = worst(out, r, variant)
        print("%s variant %d: error / bound %.3f, moves %d, f32 terms / bound %.3f" % (case_id(case), variant, w, moves,
                                                                                       float((r.f32 / r.bound[0]).max())))
        assert w <= 1.0
        assert S == 1 or w >= 0.05, "the bound is not within a factor 20 of the emulation's error: it pins nothing"
    assert float((r.f32 / r.bound[0]).max()) <= 0.25, "the bf16 terms no longer lead the bound"


@pytest.mark.parametrize("case,floor", [((1, 1, 1500, "peaked"), 150), ((3, 2, 1500, "peaked"), 800), ((3, 2, 193, "peaked"), 8),
                                        ((3, 2, 127, "peaked"), 8)], ids=lambda c: case_id(c) if isinstance(c, tuple) else None)
def test_peaked_input_takes_late_moves(case, floor):
    """measured 390, 2172, 21 and 22; the floors are well below, so that a change of the inputs cannot silently stop exercising
    the rescale with old mass that still matters"""
    B, H, S, kind = case
    q, k, v, _ = spread(case)
    _, moves = E.emulate(q, k, v, H)
    print("%s: %d moves" % (case_id(case), moves))
    assert moves >= floor


@pytest.mark.parametrize("case", [c for c in MUTANT_CASES if c[2] > 1], ids=case_id)
@pytest.mark.parametrize("mutant", ["drop_last", "double_key"])
def test_dropped_or_doubled_key_exceeds_the_bound_in_every_case(case, mutant):
    B, H, S, kind = case
    q, k, v, r = spread(case)
    out, _ = E.emulate(q, k, v, H, mutant=mutant)
    w = worst(out, r)
    print("%s %s: error / bound %.1f" % (case_id(case), mutant, w))
    assert w > (8.0 if S == 1500 else 20.0)      # measured >= 8.2 at S = 1500, >= 21 below


@pytest.mark.parametrize("mutant", ["alpha_half", "alpha_half_acc", "per_lane_stale_c"])
def test_wrong_rescale_exceeds_the_bound_where_a_row_moves(mutant):
    """alpha and the C operand act only when a row moves after the first tile: every peaked case with moves shows them (the
    per-lane decision only where a later tile follows the move: S = 127 and 192 move in their last tile)."""
    seen = 0
    for case in MUTANT_CASES:
        B, H, S, kind = case
        q, k, v, r = spread(case)
        _, moves = E.emulate(q, k, v, H)
        out, _ = E.emulate(q, k, v, H, mutant=mutant)
        w = worst(out, r)
        print("%s %s: error / bound %.1f (%d moves)" % (case_id(case), mutant, w, moves))
        if moves == 0:
            assert w <= 1.0
        elif mutant != "per_lane_stale_c" or S in (193, 1500):
            assert w > 20.0
            seen += 1
    assert seen >= (2 if mutant == "per_lane_stale_c" else 4)


def test_row_sum_of_rounded_p_has_its_own_bound():
    """see the module docstring: not a mistake the f32 row sum's bound can catch; it is the SUM_MFMA variant, and obeys that
    variant's bound"""
    big = 0.0
    for case in MUTANT_CASES:
        q, k, v, r = spread(case)
        out, _ = E.emulate(q, k, v, case[1], mutant="sum_rounded")
        assert worst(out, r, 1) <= 1.0
        big = max(big, worst(out, r, 0))
    print("row sum of the rounded P against the f32 row sum's bound: %.3f" % big)


# ---- the exact probes ------------------------------------------------------------------------------------------------------
PROBES = E.threshold_cases()


def test_selection_code_keeps_its_lead():
    c = E.code_matrix().astype(np.float64)
    g = c @ c.T
    np.fill_diagonal(g, -64)
    assert g.max() <= 44                       # measured 36: the selected key leads by >= 20 * 16 * bf16(QSCALE) = 57 log2 units
    for B, H, S in ((3, 2, 1500), (2, 5, 129)):
        q, k, v, want = E.selection_probe(B, H, S)
        assert np.array_equal(E.bf16(k), k) and np.array_equal(E.bf16(v), v)
        if S == 129:
            r = E.restate(q, k, v, H)
            assert np.abs(r.ref - want).max() <= 2.0 ** -40
            assert np.array_equal(E.emulate(q, k, v, H)[0], want)
            assert not np.array_equal(want[0, :, :64], want[1, :, :64]) and not np.array_equal(want[0, :, :64], want[0, :, 64:128])


@pytest.mark.parametrize("name,amp,kint", PROBES, ids=[p[0] for p in PROBES])
def test_probe_emulation_is_inside_the_gate_and_mutants_outside(name, amp, kint):
    B, H, S = amp.shape
    q, k, v, exact, marks = E.threshold_probe(amp, kint)
    assert np.array_equal(E.bf16(k), k) and set(np.unique(v)) <= {0.0, 1.0}
    assert all(len(set(m[m >= 0])) == (m >= 0).sum() == 64 for m in marks.reshape(-1, 64))
    sums = E.heads(exact, H).sum(axis=-1)
    assert (sums <= 1.0 + 1e-12).all() and (exact >= 0).all()
    gate = E.probe_gate(exact, S)
    out, moves = E.emulate(q, k, v, H)
    assert (np.abs(out - exact) <= gate).all()
    if S == 1500:
        return                                   # (the mutants at the two smaller S: the same paths, a tenth of the time)
    out1, _ = E.emulate(q, k, v, H, sum_rounded=True)
    assert (np.abs(out1 - exact) <= gate).all()
    # integer scores: every p is a power of two, so P = p and the two row sums agree bit for bit
    assert np.array_equal(out, out1)
    e = int(name.split("-e")[1]) if name.startswith("base") else None
    moved = moves > 0
    assert moved == (e is None or e > 8), (name, moves)
    miss = {m: int((np.abs(E.emulate(q, k, v, H, mutant=m)[0] - exact) > gate).sum())
            for m in ("drop_last", "double_key", "alpha_half", "alpha_half_acc")}
    print(name, "moves", moves, miss)
    assert miss["drop_last"] > 0 and miss["double_key"] > 0
    assert (miss["alpha_half"] > 0) == moved and (miss["alpha_half_acc"] > 0) == moved


def test_a_threshold_off_by_one_shows_in_the_move_count_not_in_the_value():
    """p = 256 kept against a move at excess 8 is the same value either way (exact powers of two): the probes pin the VALUES on
    both sides of the threshold; which side moved is the emulation's statement, checked here at 8 and 9."""
    for e, moves in ((8, 0), (9, 3 * 2 * 200)):
        kint = np.zeros((3, 2, 200), np.int64)
        for b, pos in enumerate(E.key_positions(200)):
            kint[b, 0, pos], kint[b, 1, pos + 1] = e, e
        q, k, v, exact, _ = E.threshold_probe(np.ones((3, 2, 200)), kint)
        assert E.emulate(q, k, v, 2)[1] == moves
