"""Kernel-level tests of the encoder GEMM (csrc/gemm.hip) with every epilogue and the batched row maps that turn both Conv1d
layers into implicit GEMMs, through wmdbg_gemm_mapped: every element of every returned buffer is compared with the float64
restatement of tests/enc_gemm_ref.py, and every element the kernel must not write has to keep its sentinel.

(a) exact placement: one-hot A rows, small integer weights and bias -- no rounding anywhere, so array_equal on the bits;
(b) numeric: random asymmetric operands, per element, against the DERIVED bound of enc_gemm_ref (delta = 2 K u S; half a
    bf16 ulp on bf16 outputs; GELU: 1.13 delta + 1e-6) -- no measured tolerance.
Every case runs through the four tile kernels (64, 128 double buffer, 128 pipeline, 256), which share store_tile /
store_tile_staged / resid_tile_staged: the tile-against-tile tests of test_kernels_gpu.py cannot see a mistake in those."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_gemm_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

TILES = ((64, 0), (128, 1), (128, 2), (256, 0))    # (tile, gemm128_pipe): 1 = double buffer, 2 = the 3-stage pipeline
EPI_NAMES = ("bias_bf16", "gelu_bf16", "resid_f32", "conv2_f32", "qkv_enc", "xkv", "f32")
_WORST = {}                                         # epilogue -> largest error / bound seen by the numeric tests


class Map(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_int32) for f in ("M", "N", "K", "epi")] +
                [(f, ctypes.c_int64) for f in ("a_off", "a_rpb", "a_bstride", "a_rstride", "a_elems",
                                               "c_off", "c_rpb", "c_bstride", "c_rstride", "c_elems")] +
                [(f, ctypes.c_int32) for f in ("d_model", "n_head", "seq", "seq_pad", "batch", "reserved")] +
                [("vt_elems", ctypes.c_int64)])


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.binding.Context(debug=True)
    vp = ctypes.c_void_p
    c.lib.wmdbg_gemm_mapped.argtypes = [vp, ctypes.POINTER(Map), vp, vp, vp, vp, vp, vp]
    c.lib.wmdbg_set_gemm_tile.argtypes = [ctypes.c_int]
    c.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    c.lib.wm_last_error.restype = ctypes.c_char_p
    lay = (ctypes.c_int32 * 4)()
    assert c.lib.wmdbg_gemm_map_layout(lay) == 0
    assert list(lay) == [ctypes.sizeof(Map), Map.a_off.offset, Map.d_model.offset, Map.vt_elems.offset], list(lay)
    yield c
    c.lib.wmdbg_set_gemm_tile(0)
    c.lib.wmdbg_set_tuning(b"reset", 0)
    c.close()
    for k in sorted(_WORST):          # (shown with -s) largest |got - ref| / bound per epilogue; the bound is derived, not measured
        print("error / bound, %-12s %.4f" % (k, _WORST[k]))


def to_map(g):
    return Map(**{f: getattr(g, f) for f in R.Geom.FIELDS})


def run(ctx, g, A, W, bias, pos=None, C0=None):
    """One launch of the current tile: (C, vt) as the hook returns them (widened f32), vt None without EPI_QKV_ENC."""
    C = np.zeros(g.c_elems, np.float32) if C0 is None else np.array(C0, np.float32)
    vt = np.zeros(g.vt_elems, np.float32) if g.epi == R.EPI_QKV_ENC else None
    A, W, bias = (np.ascontiguousarray(a, np.float32) for a in (A, W, bias))
    m = to_map(g)
    st = ctx.lib.wmdbg_gemm_mapped(ctx.handle, ctypes.byref(m), P(A), P(W), P(bias), P(pos), P(C), P(vt))
    assert st == 0, ctx.lib.wm_last_error()
    return C, vt


def tiles_of(g):
    return [t for t in TILES if t[0] != 256 or g.K >= 128]


def every_tile(ctx, g):
    for tile, pipe in tiles_of(g):
        assert ctx.lib.wmdbg_set_gemm_tile(tile) == 0
        assert ctx.lib.wmdbg_set_tuning(b"gemm128_pipe", pipe) == 0
        yield tile, pipe


@pytest.mark.parametrize("case", R.exact_cases(), ids=lambda c: c[0])
def test_exact_placement(ctx, case):
    """(a) Every output element in its place and nothing anywhere else, bit for bit."""
    _, g = case
    A, W, bias, C0 = R.exact_operands(g)
    vals, _ = R.values(g, A, W, bias, C0=C0)
    want_C, want_vt = R.exact_outputs(g, vals, C0)
    try:
        for tile in every_tile(ctx, g):
            C, vt = run(ctx, g, A, W, bias, C0=C0)
            bad = np.flatnonzero(C.view(np.uint32) != want_C)
            assert bad.size == 0, (tile, "C", bad.size, bad[:8], C[bad[:8]], want_C[bad[:8]].view(np.float32))
            if vt is not None:
                bad = np.flatnonzero(vt.view(np.uint32) != want_vt)
                assert bad.size == 0, (tile, "vt", bad.size, bad[:8], vt[bad[:8]], want_vt[bad[:8]].view(np.float32))
                pad = vt.view(np.uint32).reshape(-1, g.seq_pad)[:, 16 * ((g.seq + 15) // 16):]
                assert (pad == R.SENT_BF16).all()                       # the pad columns hold the sentinel
    finally:
        ctx.lib.wmdbg_set_gemm_tile(0)
        ctx.lib.wmdbg_set_tuning(b"reset", 0)


@pytest.mark.parametrize("case", R.numeric_cases(), ids=lambda c: c[0])
def test_numeric_per_element(ctx, case):
    """(b) Every element within the derived bound of its float64 value; sentinels everywhere else."""
    name, g = case
    A, W, bias, pos, C0 = R.random_operands(g, seed=sum(name.encode()))
    ref, S = R.values(g, A, W, bias, pos=pos, C0=C0)
    try:
        for tile in every_tile(ctx, g):
            C, vt = run(ctx, g, A, W, bias, pos=pos, C0=C0)
            if g.epi == R.EPI_RESID_F32:                                # in / out: what is not a destination keeps its old bits
                ci, _ = R.dest_index(g)
                keep = np.ones(g.c_elems, bool)
                keep[ci.ravel()] = False
                assert np.array_equal(C.view(np.uint32)[keep], C0.view(np.uint32)[keep]), tile
            worst = R.scatter_check(g, C, vt, ref, S)
            print("%s tile %s: error / bound = %.4f" % (name, tile, worst))
            key = EPI_NAMES[g.epi]
            _WORST[key] = max(_WORST.get(key, 0.0), worst)
            assert worst <= 1.0, (tile, worst)
    finally:
        ctx.lib.wmdbg_set_gemm_tile(0)
        ctx.lib.wmdbg_set_tuning(b"reset", 0)


def _bad_maps():
    ok = R.batched_c(R.plain(150, 64, 128, R.EPI_F32), 50)
    q = R.qkv_geom(128, 2, 37, 3, 128)
    x = R.xkv_geom(128, 2, 37, 3, 128)
    c1 = R.R_conv1(80, 100, 3, 64, R.EPI_BIAS_BF16)
    return [
        ("A row past a_elems + slack", ok.copy(a_elems=ok.a_elems - 256), b"A row"),
        ("conv1 window past the slack", c1.copy(a_elems=c1.a_elems - 160), b"A row"),
        ("A map not aligned", ok.copy(a_off=4, a_elems=ok.a_elems + 8), b"aligned"),
        ("K not a multiple of 64", ok.copy(K=96), b"problem size"),
        ("C row past c_elems", ok.copy(c_elems=ok.c_elems - 1), b"C row"),
        ("C rows overlap: c_rstride < N", ok.copy(c_rstride=56, c_off=56, c_bstride=51 * 56), b"overlap"),
        ("C batches overlap", ok.copy(c_bstride=49 * 64), b"overlap"),
        ("C map not aligned for the staged stores", ok.copy(c_off=66, c_elems=ok.c_elems + 8), b"aligned"),
        ("bad epilogue", ok.copy(epi=7), b"epilogue"),
        ("conv2 without pos", ok.copy(epi=R.EPI_CONV2_F32), b"pos"),
        ("xkv: M != batch * seq", x.copy(batch=2), b"batch * seq"),
        ("xkv: N != 2 d", x.copy(d_model=64, n_head=1), b"2 * d_model"),
        ("xkv: d != 64 H", x.copy(n_head=3), b"64 * n_head"),
        ("xkv: c_elems", x.copy(c_elems=x.c_elems - 64), b"c_elems"),
        ("qkv: M != batch * seq", q.copy(seq=36), b"batch * seq"),
        ("qkv: N != 3 d", q.copy(N=2 * 128), b"3 * d_model"),
        ("qkv: seq_pad % 16", q.copy(seq_pad=40, vt_elems=3 * 2 * 64 * 40), b"seq_pad"),
        ("qkv: seq_pad < seq", q.copy(seq_pad=32, vt_elems=3 * 2 * 64 * 32), b"seq_pad"),
        ("qkv: vt_elems", q.copy(vt_elems=q.vt_elems - 64), b"vt_elems"),
        ("qkv: C row narrower than 2 d", q.copy(c_rstride=128), b"overlap"),
    ]


@pytest.mark.parametrize("case", _bad_maps(), ids=lambda c: c[0])
def test_rejected_maps_launch_nothing(ctx, case):
    """The hook validates every address on the host: a map that would take the kernel outside a buffer is WM_ERR_INVALID with
    the reason in wm_last_error, and the output buffers come back untouched (nothing was launched or copied)."""
    _, g, word = case
    n = 1 << 16
    A = np.zeros(max(n, g.a_elems), np.float32)
    W = np.zeros(max(n, g.N * g.K), np.float32)
    bias = np.zeros(max(n, g.N), np.float32)
    C = np.full(max(n, g.c_elems), 7.0, np.float32)
    vt = np.full(max(n, g.vt_elems), 7.0, np.float32)
    m = to_map(g)
    st = ctx.lib.wmdbg_gemm_mapped(ctx.handle, ctypes.byref(m), P(A), P(W), P(bias), None, P(C), P(vt))
    assert st == 1                                                          # WM_ERR_INVALID
    assert word in ctx.lib.wm_last_error(), ctx.lib.wm_last_error()
    assert (C == 7.0).all() and (vt == 7.0).all()
