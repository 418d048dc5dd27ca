"""tests/layernorm_ref.py held to its conditions, on the CPU: the restatement equals torch's float64 layer_norm; an f32 emulation of
the kernel's order stays inside the derived bound on every input of the GPU tests; each value-only mistake exceeds it there.

Measured (largest error / bound over all 73 shapes): normal 0.56, mean = 30 x std 0.17, outlier column 0.82, constant rows 0.12.
Mutants, shapes (of 73) at which the largest error / bound is over 1: divisor d - 1 and a dropped last quad 73 on every
non-constant kind (smallest 45); one-pass variance 72 on mean = 30 x std (up to 19; constant rows give a negative variance);
eps 1e-6 62 on the normal kind (the rows at scale 0.3 and 0.03; up to 22528); one quad too many 55 on every non-constant kind
(every shape with a next row or a non-zero quad behind it in the register file's range)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layernorm_ref as L   # noqa: E402

CASES = L.cases()


def ratio(y, ref, bound):
    with np.errstate(invalid="ignore"):
        r = np.abs(y.astype(np.float64) - ref) / bound
    return float(np.where(np.isfinite(r), r, np.inf).max())


def test_shapes_cover_every_instantiation_boundary_and_row_tail():
    assert [L.maxp(d) for d in (4, 256, 260, 768, 772, 1280)] == [1, 1, 3, 3, 5, 5]
    assert {r % 4 for r in L.ROWS} == {0, 1, 2, 3} and (1500, 384) in CASES and len(CASES) == 73
    for d in (252, 764, 1276):                      # the last lane of the last register holds no quad
        assert d // 4 == L.maxp(d) * 64 - 1


@pytest.mark.parametrize("kind", L.KINDS)
def test_restatement_and_emulation(kind):
    big = 0.0
    for rows, d in CASES:
        g, b = L.params(d)
        x = L.inputs(rows, d, kind)
        y, bound = L.restate(x, g, b)
        t = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (d,), torch.from_numpy(g).double(),
                                           torch.from_numpy(b).double(), 1e-5).numpy()
        assert np.abs(t - y).max() <= 1e-9 * max(1.0, np.abs(y).max())
        if kind == "constant":
            assert np.abs(y - b).max() <= 1e-9
        if kind == "mean30":
            assert (np.abs(x.mean(axis=1)) >= 15 * x.std(axis=1)).all()       # (30 x the population's; a row's own varies)
        if kind == "outlier":
            assert (np.abs(x).max(axis=1) >= 1e3 * np.median(np.abs(x), axis=1)).all() or d == 4
        r = ratio(L.emulate(x, g, b), y, bound)
        assert r <= 1.0, (rows, d, r)
        big = max(big, r)
    print("%s: emulation error / bound %.3f" % (kind, big))
    assert big >= 0.05, "the bound is not within a factor 20 of the emulation's error: it pins nothing"


def test_mean_error_scales_with_the_mean_of_abs_x():
    """the same spread at 1000 x the mean: the bound of a centred element grows with sum |x| / d"""
    d = 384
    g, b = np.ones(d, np.float32), np.zeros(d, np.float32)
    z = np.random.default_rng(1).standard_normal((4, d))
    b0 = L.restate(z.astype(np.float32), g, b)[1]
    b1 = L.restate((z + 1000.0).astype(np.float32), g, b)[1]
    assert np.median(b1 / b0) > 100
    x = (z + 1000.0).astype(np.float32)
    assert ratio(L.emulate(x, g, b), *L.restate(x, g, b)) <= 1.0


@pytest.mark.parametrize("mutant,kind,least", [("one_pass", "mean30", 70), ("eps_1e-6", "normal", 55), ("divisor_d-1", "normal", 73),
                                               ("divisor_d-1", "mean30", 73), ("divisor_d-1", "outlier", 73),
                                               ("last_quad_dropped", "normal", 73), ("last_quad_dropped", "constant", 73),
                                               ("reads_one_quad_more", "normal", 50), ("reads_one_quad_more", "mean30", 50)])
def test_mutant_exceeds_the_bound(mutant, kind, least):
    over = 0
    for rows, d in CASES:
        g, b = L.params(d)
        x = L.inputs(rows, d, kind)
        y, bound = L.restate(x, g, b)
        with np.errstate(invalid="ignore"):
            over += ratio(L.emulate(x, g, b, mutant), y, bound) > 1.0
    print("%s on %s: over the bound at %d of %d shapes" % (mutant, kind, over, len(CASES)))
    assert over >= least


def test_one_quad_more_shows_at_the_instantiation_boundaries():
    """d = 260 and 772 run the next instantiation: a bound `idx <= np` there reads the next row's first quad"""
    for d in (252, 260, 764, 772, 1276):
        g, b = L.params(d)
        x = L.inputs(5, d, "normal")
        y, bound = L.restate(x, g, b)
        assert ratio(L.emulate(x, g, b, "reads_one_quad_more"), y, bound) > 1.0
