"""layernorm_kernel (csrc/enc_kernels.hip) at kernel level, through wmdbg_layernorm: every element of the f32 output within the
bound derived from the kernel's order (tests/layernorm_ref.py, held to its conditions by test_layernorm_ref_cpu.py), at both
sides of every MAXP instantiation boundary and every row tail, on inputs with a large mean, an outlier column and constant
rows; the bf16 output bit-equal to RNE of the same launch's f32 output; and the three ways the product launches it -- bf16
only, f32 only, both -- giving the same bits."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layernorm_ref as L   # noqa: E402

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
SENT = np.uint32(0x7fc0dead)
_WORST = {}


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_layernorm.argtypes = [vp, vp, vp, vp, ip, ip, vp, vp]
    c.lib.wm_last_error.restype = ctypes.c_char_p
    yield c
    c.close()
    for k in sorted(_WORST):               # (shown with -s) largest |got - ref| / bound per input kind
        print("error / bound, layernorm %-9s %.4f" % (k, _WORST[k]))


def P(a):
    return None if a is None else a.ctypes.data_as(vp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sentinels(shape):
    return np.full(shape, SENT, np.uint32).view(np.float32)


def launch(dbg, x, g, b, f32=True, bf16=True):
    """-> (status, f32 output or None, bf16 output widened or None); outputs start as sentinels"""
    rows, d = x.shape
    of = sentinels(x.shape) if f32 else None
    ob = sentinels(x.shape) if bf16 else None
    st = dbg.lib.wmdbg_layernorm(dbg.handle, P(np.ascontiguousarray(x)), P(g), P(b), rows, d, P(of), P(ob))
    return st, of, ob


@pytest.mark.parametrize("rows,d", L.cases(), ids=lambda v: str(v))
def test_every_element_every_output_form(dbg, rows, d):
    g, b = L.params(d)
    for kind in L.KINDS:
        x = L.inputs(rows, d, kind)
        y, bound = L.restate(x, g, b)
        st, of, ob = launch(dbg, x, g, b)
        assert st == 0, dbg.lib.wm_last_error()
        ratio = np.abs(of.astype(np.float64) - y) / bound
        assert np.isfinite(ratio).all(), (kind, "an element is not finite (never written?)")
        worst = float(ratio.max())
        print("rows %d d %d %s: error / bound = %.4f" % (rows, d, kind, worst))
        _WORST[kind] = max(_WORST.get(kind, 0.0), worst)
        assert worst <= 1.0, (kind, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
        assert np.array_equal(bits(ob), bits(L.bf16(of))), (kind, "bf16 output is not RNE of the f32 output")
        st1, of1, none1 = launch(dbg, x, g, b, bf16=False)          # the f32 debug path's launch
        st2, none2, ob2 = launch(dbg, x, g, b, f32=False)           # the encoder layers' launch
        assert st1 == 0 and st2 == 0 and none1 is None and none2 is None
        assert np.array_equal(bits(of1), bits(of)) and np.array_equal(bits(ob2), bits(ob)), kind


@pytest.mark.parametrize("d", [6, 1284])
def test_unsupported_width_is_refused_and_nothing_is_written(dbg, d):
    x = np.ones((3, d), np.float32)
    g, b = np.ones(d, np.float32), np.zeros(d, np.float32)
    st, of, ob = launch(dbg, x, g, b)
    assert st == 1 and b"layernorm" in dbg.lib.wm_last_error()
    assert (bits(of) == SENT).all() and (bits(ob) == SENT).all()
    st, of, ob = launch(dbg, np.ones((3, 8), np.float32), np.ones(8, np.float32), np.zeros(8, np.float32))   # ... and the hook still works
    assert st == 0 and np.array_equal(of, np.zeros((3, 8), np.float32))
