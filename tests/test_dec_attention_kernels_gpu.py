"""Kernel-level GPU tests of the decode attention family (csrc/dec_kernels.hip: dec_xrows_attn_kernel, dec_rows_attn_kernel,
dec_xcand_attn_kernel, dec_xattn_fq_kernel, dec_attn_combine_kernel) and of the encoder attention, on inputs whose right answer
is EXACT, every launch form driven alone through wmdbg_dec_attention_form (include/whisper_mi355x_debug.h), every key position
covered.  The probes, their f64 reference and the row geometry are tests/dec_attn_ref.py; tests/test_dec_attn_ref_cpu.py shows
what each probe rejects.  Every K and V element outside a pair's key range is NaN in every test below.

Each test asserts the plan record of the launch it means to test (variant, grid, warm-up tiles): a tuning knob that silently
stopped selecting a kernel would otherwise leave its test running another one.  The variants by test:
  DAV_STREAM (one round, several rounds with an uneven tail, (pair, split) grids, short-lived), DAV_FLAT, DAV_FLAT_DEEP_C,
  DAV_FLAT_DEEP_NT: test_cross_variants_exact; DAV_SELF: test_self_attention_every_key_count; DAV_SELF_OFF:
  test_ragged_rows; DAV_SELF_PANEL / DAV_SELF_OFF_PANEL: test_panels_count_every_key; DAV_CAND / DAV_CAND_FLAT:
  test_candidate_groups; DAV_FQ: test_fused_query.
Key positions: test_cross_all_1536_keys_counted covers 0 .. 1535, test_self_all_448_keys_counted 0 .. 447.

The spread numeric case (dec_attn_ref.spread_case) is gated per element, |out - ref| <= 2^-8 |ref| + 2^-12 max|v|; the numpy
f32 restatement with another summation order sits at 0.43 - 0.62 of that gate (test_dec_attn_ref_cpu.py).

MEASURED on the MI355X (worst |out - ref| / gate of a launch; every exact probe passes on every variant, no kernel changed):
  cross: stream one round / (pair, split) grids 2, 4, 8 / flat / deep cacheable, 6 pairs   0.398 (one figure: the same bits)
         stream 40 pairs in 5 rounds 0.662, 37 pairs with an uneven tail 0.616, short-lived 10 pairs 0.544, deep NT 10 pairs 0.544
  self: constant key count 0.526, device position 0.526;  candidate groups: flat 0.573, short-lived 0.573
  fused query, against the f64 attention over the GPU's own query: 0.749 / 0.624 / 0.648 / 0.737 / 0.712 / 0.753 (the table's order);
         against the all-f64 chain with the LN-GEMV tolerance carried: 0.001 - 0.002 of a gate that the carried term dominates
         (D = 0.41 - 0.49 in score units, i.e. up to e^(2 D) - 1 = 1.6 max|v|): that gate can only catch a gross error, the first can
         catch a subtle one, and the bit-equality with the two launches ties the fused kernel to the tested GEMV and stream kernels.
"""
import contextlib
import ctypes
import types

import numpy as np
import pytest

import dec_attn_ref as A

pytestmark = pytest.mark.gpu

vp, ip, i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32
WM_ERR_INVALID = 1
SENT16 = 0x7fc5                          # WMDBG_SENTINEL_BF16
DE_Q = 1                                 # DecEpi
(DAV_STREAM, DAV_FLAT, DAV_FLAT_DEEP_C, DAV_FLAT_DEEP_NT, DAV_SELF, DAV_SELF_OFF, DAV_SELF_PANEL, DAV_CAND, DAV_CAND_FLAT, DAV_FQ,
 DAV_SELF_OFF_PANEL) = range(11)
# the plan record (wmdbg_dec_attn_plan's out)
P_STATUS, P_VARIANT, P_SPW, P_GRID_X, P_GRID_Y, P_BLOCK, P_LDS, P_NWG, P_WARM, P_TILE_BYTES, P_A, P_B, P_C, P_COMBINE, P_RULE = range(15)

CODE = A.code_matrix()


class Attn(ctypes.Structure):
    """struct wmdbg_attn"""
    _fields_ = [(n, i32) for n in ("form", "B", "C", "N", "H", "T", "n_keys", "nsplit", "pos", "n_live", "short_lived", "warm_rows",
                                   "warm_k", "K")] + \
               [(n, vp) for n in ("off", "live_rows", "q", "k", "v", "x", "ln_g", "ln_b", "Wq", "bias", "out", "mean_out")] + \
               [("plan", i32 * 16)]


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    lib = c.lib
    lib.wmdbg_dec_attention_form.argtypes = [vp, ctypes.POINTER(Attn)]
    lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ip]
    lib.wmdbg_dec_attn_plan.argtypes = [vp, ip, vp]
    lib.wmdbg_dec_gemv_ln.argtypes = [vp, ip] + [vp] * 5 + [ip] * 7 + [vp] * 8
    lib.wmdbg_dec_attention_cand.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    lib.wmdbg_dec_attention_cand_shared.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    lib.wmdbg_dec_self_attention_panel.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    lib.wmdbg_dec_self_attention_panel_off.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    lib.wmdbg_enc_attention.argtypes = [vp, vp, vp, vp, ip, ip, ip, vp]
    lay = (i32 * 4)()      # the ctypes restatement above against the header's struct
    assert lib.wmdbg_attn_layout(lay) == 0
    assert list(lay) == [ctypes.sizeof(Attn), Attn.off.offset, Attn.out.offset, Attn.plan.offset], list(lay)
    yield c
    lib.wmdbg_set_tuning(b"reset", 0)
    c.close()


@contextlib.contextmanager
def tuning(dbg, **knobs):
    """every use of wmdbg_set_tuning: set inside try, "reset" in finally"""
    try:
        for key, val in knobs.items():
            assert dbg.lib.wmdbg_set_tuning(key.encode(), val) == 0
        yield
    finally:
        dbg.lib.wmdbg_set_tuning(b"reset", 0)


def P(a):
    return None if a is None else a.ctypes.data_as(vp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def err_msg(dbg):
    return dbg.lib.wm_last_error().decode("utf-8", "replace")


def attn(dbg, form, q, k, v, n_keys=0, nsplit=1, pos=-1, off=None, live=None, short=0, warm=(0, 0), N=0, fq=None, expect_ok=True,
         T=None):
    """one wmdbg_dec_attention_form call.  k / v [entries][H][T][64]; q [rows][H * 64] (None for form 2, whose query side is
    fq = (x, ln_g, ln_b, Wq, bias)); N: candidates per window (form 1).  -> rc, out [rows][H * 64], pad (the rows behind), mean, plan"""
    E, H = k.shape[0], k.shape[1]
    T = T or k.shape[2]
    rows = fq[0].shape[0] if form == 2 else q.shape[0]
    rpad = -(-rows // 16) * 16
    io = Attn()
    io.form, io.H, io.T, io.n_keys, io.nsplit, io.pos, io.short_lived = form, H, T, n_keys, nsplit, pos, short
    io.warm_rows, io.warm_k = warm
    if form == 1:
        io.C, io.N = E, N
    else:
        io.B = rows
    keep = [np.ascontiguousarray(a, np.float32) for a in (k, v)]
    io.k, io.v = P(keep[0]), P(keep[1])
    if form == 2:
        keep += [np.ascontiguousarray(a, np.float32) if a is not None else None for a in fq]
        io.x, io.ln_g, io.ln_b, io.Wq, io.bias = (P(a) for a in keep[2:7])
        io.K = fq[0].shape[1]
    else:
        keep.append(np.ascontiguousarray(q, np.float32))
        io.q = P(keep[-1])
    if off is not None:
        keep.append(np.ascontiguousarray(off, np.int32))
        io.off = P(keep[-1])
    if live is not None:
        keep.append(np.ascontiguousarray(list(live) + [0], np.int32))
        io.live_rows, io.n_live = P(keep[-1]), len(live)
    out = np.zeros((rpad, H * 64), np.float32)
    mean = np.zeros(rows, np.float32)
    io.out, io.mean_out = P(out), P(mean)
    rc = dbg.lib.wmdbg_dec_attention_form(dbg.handle, ctypes.byref(io))
    if expect_ok:
        assert rc == 0, err_msg(dbg)
    return types.SimpleNamespace(rc=rc, out=out[:rows], pad=out[rows:], full=out, mean=mean, plan=list(io.plan))


def cross_plan_check(r, variant, pairs, **want):
    assert r.plan[P_STATUS] == 0 and r.plan[P_VARIANT] == variant, r.plan
    for name, val in want.items():
        assert r.plan[globals()["P_" + name.upper()]] == val, (name, val, r.plan)
    assert np.all(bits(r.pad) == SENT16 << 16), "a pad row was written"


# ------------------------------------------------------------------ probe -> launch tensors
def pair_major(rows, H, q, k, v):
    """pair p = row * H + head of the builders -> the hooks' layouts"""
    return A.heads(q, rows, H), A.heads(k, rows, H), A.heads(v, rows, H)


def selection_keys(n, NS, pairs):
    """`pairs` selected keys: the boundary keys of n first, then keys spread over the range"""
    ks = A.boundary_keys(n, NS)
    extra = [int(x) for x in np.random.default_rng(n + pairs).integers(0, n, 4 * pairs)]
    return (ks + extra)[:pairs] if pairs >= len(ks) else [ks[(i * 5) % len(ks)] for i in range(pairs)]


def exact_probes(launch, rows, H, T, n, NS, what):
    """the counting, selection and two-peak probes over keys [0, n) through launch(q, k, v) -> out [rows][H * 64]"""
    pairs = rows * H
    q, k, v, marks = A.counting_probe(pairs, T, 0, n - 1, NS)
    out = launch(*pair_major(rows, H, q, k, v))
    bad = A.counting_check(out.reshape(pairs, 64), marks, n)
    assert not bad, (what, "counting: (pair, column, got), want 1/%d or 0" % n, bad[:8])
    sel = selection_keys(n, NS, pairs)
    q, k, v, want = A.selection_probe(CODE, sel, T, 0, n - 1)
    out = launch(*pair_major(rows, H, q, k, v)).reshape(pairs, 64)
    miss = [(p, sel[p]) for p in range(pairs) if not np.array_equal(bits(out[p]), bits(want[p]))]
    assert not miss, (what, "selection: (pair, selected key) whose output is not v[key] bit for bit", miss[:8])
    pk = A.two_peak_pairs(CODE, n, NS)
    if pk:
        pk = [pk[i % len(pk)] for i in range(pairs)]
        q, k, v, want = A.two_peak_probe(CODE, pk, T, n)
        out = launch(*pair_major(rows, H, q, k, v)).reshape(pairs, 64)
        miss = [(p, pk[p]) for p in range(pairs) if not np.array_equal(bits(out[p]), bits(want[p]))]
        assert not miss, (what, "two-peak: (pair, (a, b)) whose output is not (v[a] + v[b]) / 2 bit for bit", miss[:8])
    return marks


# ------------------------------------------------------------------ cross-attention variants (form 0)
# name -> (B, H, T, nsplit, knobs, short_lived, variant, plan fields)
def _flat(pairs):
    units = pairs * 8
    w = min(4, max(1, -(-units // 256)))
    return dict(block=w * 64, grid_x=-(-units // w), grid_y=1, combine=pairs)


CROSS = {
    "stream_one_round": (3, 2, 1500, 1, {}, 0, DAV_STREAM, dict(nwg=6, grid_x=6, grid_y=1, block=512, combine=0)),
    "stream_5_rounds_40_pairs": (20, 2, 1500, 1, dict(xattn_wgs=8), 0, DAV_STREAM, dict(nwg=8, grid_x=8, grid_y=1, block=512)),
    "stream_uneven_tail_37_pairs": (37, 1, 1500, 1, dict(xattn_wgs=8), 0, DAV_STREAM, dict(nwg=8, grid_x=8, grid_y=1, block=512)),
    "stream_grid_split_2": (3, 2, 1500, 2, dict(xattn_no_flat=1), 0, DAV_STREAM, dict(nwg=6, grid_x=6, grid_y=2, block=256, combine=6)),
    "stream_grid_split_4": (3, 2, 1500, 4, dict(xattn_no_flat=1), 0, DAV_STREAM, dict(nwg=6, grid_x=6, grid_y=4, block=128, combine=6)),
    "stream_grid_split_8": (3, 2, 1500, 8, dict(xattn_no_flat=1), 0, DAV_STREAM, dict(nwg=6, grid_x=6, grid_y=8, block=64, combine=6)),
    "stream_short_lived": (5, 2, 1500, 1, dict(xattn_wgs=4), 1, DAV_STREAM, dict(nwg=10, grid_x=10, grid_y=1, block=512)),
    "flat_6_pairs": (3, 2, 1500, 8, dict(xattn_no_deep=1), 0, DAV_FLAT, _flat(6)),
    "flat_40_pairs": (20, 2, 1500, 8, dict(xattn_no_deep=1), 0, DAV_FLAT, _flat(40)),
    "flat_65_pairs": (13, 5, 600, 8, dict(xattn_no_deep=1), 0, DAV_FLAT, _flat(65)),
    "deep_c_6_pairs": (3, 2, 1500, 8, {}, 0, DAV_FLAT_DEEP_C, _flat(6)),
    "deep_c_40_pairs": (20, 2, 300, 4, {}, 0, DAV_FLAT_DEEP_C, _flat(40)),
    "deep_c_65_pairs": (13, 5, 190, 2, {}, 0, DAV_FLAT_DEEP_C, _flat(65)),
    "deep_nt_10_pairs": (5, 2, 1500, 8, {}, 0, DAV_FLAT_DEEP_NT, _flat(10)),       # 3750 KiB of cache: more than 3200
    "deep_nt_40_pairs": (20, 2, 1500, 8, {}, 0, DAV_FLAT_DEEP_NT, _flat(40)),
    "deep_nt_65_pairs": (13, 5, 1500, 8, {}, 0, DAV_FLAT_DEEP_NT, _flat(65)),
}


def test_the_flat_deal_has_1_2_and_3_waves_and_idle_waves_behind_the_last_unit():
    assert [_flat(p)["block"] // 64 for p in (6, 40, 65)] == [1, 2, 3]
    assert _flat(65)["grid_x"] * 3 > 65 * 8          # 174 workgroups of 3 waves for 520 units: two waves find no unit


@pytest.mark.parametrize("name", list(CROSS))
def test_cross_variants_exact(dbg, name):
    B, H, T, nsplit, knobs, short, variant, want = CROSS[name]
    with tuning(dbg, **knobs):
        def launch(q, k, v):
            r = attn(dbg, 0, q, k, v, n_keys=T, nsplit=nsplit, short=short)
            cross_plan_check(r, variant, B * H, **want)
            return r.out
        exact_probes(launch, B, H, T, T, A.NS_CROSS, name)


CROSS_COUNTS = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 437, 1279, 1280, 1281, 1499, 1500]


@pytest.mark.parametrize("n", CROSS_COUNTS)
def test_cross_every_key_count(dbg, n):
    """T = 1500: the counting probe through STREAM and through the deep flat kernel (6 pairs: DAV_FLAT_DEEP_C), the selection
    probe at the count's own boundary keys (16 pairs) through both."""
    T = 1500
    for nsplit, variant in ((1, DAV_STREAM), (8, DAV_FLAT_DEEP_C)):
        q, k, v, marks = A.counting_probe(6, T, 0, n - 1, A.NS_CROSS)
        r = attn(dbg, 0, *pair_major(3, 2, q, k, v), n_keys=n, nsplit=nsplit)
        cross_plan_check(r, variant, 6)
        bad = A.counting_check(r.out.reshape(6, 64), marks, n)
        assert not bad, (n, nsplit, bad[:8])
    sel = A.boundary_keys(n, A.NS_CROSS)
    sel = [sel[i % len(sel)] for i in range(16)]
    q, k, v, want = A.selection_probe(CODE, sel, T, 0, n - 1)
    for nsplit, variant in ((1, DAV_STREAM), (8, DAV_FLAT_DEEP_NT)):     # 16 pairs at T = 1500 are 6000 KiB: the NT instantiation
        r = attn(dbg, 0, *pair_major(8, 2, q, k, v), n_keys=n, nsplit=nsplit)
        cross_plan_check(r, variant, 16)
        assert np.array_equal(bits(r.out.reshape(16, 64)), bits(want)), (n, nsplit, sel)


def test_cross_all_1536_keys_counted(dbg):
    """T = n_keys = WM_ATT_MAXK = 1536: six full blocks, the last row of the deep kernel's up-front loads; 24 pairs mark every key
    once.  STREAM, the (pair, split) grid, DAV_FLAT and both deep instantiations (24 pairs x 1536 rows are 9216 KiB: NT; 6 pairs: C)."""
    T = n = A.ATT_MAXK
    q, k, v, marks = A.counting_probe(24, T, 0, n - 1, A.NS_CROSS)
    assert sorted(marks[marks >= 0].tolist()) == list(range(1536))
    qkv = pair_major(12, 2, q, k, v)
    for nsplit, knobs, variant in ((1, {}, DAV_STREAM), (4, dict(xattn_no_flat=1), DAV_STREAM), (8, dict(xattn_no_deep=1), DAV_FLAT),
                                   (8, {}, DAV_FLAT_DEEP_NT)):
        with tuning(dbg, **knobs):
            r = attn(dbg, 0, *qkv, n_keys=n, nsplit=nsplit)
        cross_plan_check(r, variant, 24)
        bad = A.counting_check(r.out.reshape(24, 64), marks, n)
        assert not bad, (nsplit, knobs, bad[:8])
    for part in range(4):       # ... and the cacheable deep kernel: the same 24 pairs, 6 at a launch
        sl = slice(6 * part, 6 * part + 6)
        r = attn(dbg, 0, *pair_major(3, 2, q[sl], k[sl], v[sl]), n_keys=n, nsplit=8)
        cross_plan_check(r, DAV_FLAT_DEEP_C, 6)
        assert not A.counting_check(r.out.reshape(6, 64), marks[sl], n), part
    exact_probes(lambda q, k, v: attn(dbg, 0, q, k, v, n_keys=n, nsplit=1).out, 3, 2, T, n, A.NS_CROSS, "1536 keys, stream")
    exact_probes(lambda q, k, v: attn(dbg, 0, q, k, v, n_keys=n, nsplit=8).out, 3, 2, T, n, A.NS_CROSS, "1536 keys, deep")


def test_cross_position_from_device_memory(dbg):
    """dec_xrows_attn_kernel also takes its key count as *pos_ptr + 1 (n_keys_const is then the row clamp only)."""
    T, n = 1500, 437
    q, k, v, want = A.selection_probe(CODE, selection_keys(n, 8, 6), T, 0, n - 1)
    r = attn(dbg, 0, *pair_major(3, 2, q, k, v), n_keys=n, pos=n - 1)
    cross_plan_check(r, DAV_STREAM, 6)
    assert np.array_equal(bits(r.out.reshape(6, 64)), bits(want))


# ------------------------------------------------------------------ the causal self-attention (form 3)
SELF_COUNTS = list(range(1, 131)) + [255, 256, 257, 447, 448]


@pytest.mark.parametrize("from_device", [0, 1])
def test_self_attention_every_key_count(dbg, from_device):
    """DAV_SELF at T = 448, B, H = 2, 2, every key count 1 .. 130 and 255, 256, 257, 447, 448: the counting probe and the selection
    probe (four of the count's boundary keys, rotating), the key count once a constant and once *pos_ptr + 1 with off == NULL."""
    T, B, H = 448, 2, 2
    for n in SELF_COUNTS:
        kw = dict(pos=n - 1, n_keys=0) if from_device else dict(n_keys=n)
        q, k, v, marks = A.counting_probe(4, T, 0, n - 1, A.NS_SELF)
        r = attn(dbg, 3, *pair_major(B, H, q, k, v), **kw)
        cross_plan_check(r, DAV_SELF, 4, grid_x=4, block=256, warm=0)
        bad = A.counting_check(r.out.reshape(4, 64), marks, n)
        assert not bad, (n, bad[:8])
        ks = A.boundary_keys(n, A.NS_SELF)
        sel = [ks[(n + i * 3) % len(ks)] for i in range(4)]
        q, k, v, want = A.selection_probe(CODE, sel, T, 0, n - 1)
        r = attn(dbg, 3, *pair_major(B, H, q, k, v), **kw)
        assert np.array_equal(bits(r.out.reshape(4, 64)), bits(want)), (n, sel)


@pytest.mark.parametrize("from_device", [0, 1])
def test_self_all_448_keys_counted(dbg, from_device):
    """8 pairs mark every key 0 .. 447 once; all boundary keys selected; the two-peak pairs at 130 and 448 keys."""
    T = n = 448
    def launch(count):
        kw = dict(pos=count - 1, n_keys=0) if from_device else dict(n_keys=count)
        return lambda q, k, v: attn(dbg, 3, q, k, v, **kw).out
    marks = exact_probes(launch(n), 4, 2, T, n, A.NS_SELF, "self 448")
    assert sorted(marks[marks >= 0].tolist()) == list(range(448))
    exact_probes(launch(130), 4, 4, T, 130, A.NS_SELF, "self 130")


def ragged_probe(kind, T, H, lo, hi):
    """per-row key ranges [lo[b], hi[b]]: q [B][H * 64], k, v [B][H][T][64], and per row what the check needs"""
    qs, ks, vs, wants = [], [], [], []
    for b in range(len(lo)):
        n = hi[b] - lo[b] + 1
        if kind == "counting":
            q, k, v, w = A.counting_probe(H, T, lo[b], hi[b], A.NS_SELF, seed=b)
        else:
            ks_b = A.boundary_keys(n, A.NS_SELF)
            q, k, v, w = A.selection_probe(CODE, [ks_b[(b + 3 * h) % len(ks_b)] for h in range(H)], T, lo[b], hi[b])
        qs.append(q.reshape(H * 64)); ks.append(k); vs.append(v); wants.append(w)
    return np.stack(qs), np.stack(ks), np.stack(vs), wants


def test_ragged_rows(dbg):
    """DAV_SELF_OFF at position 200 of T = 448 with offsets before (0, 57, 73), just before (199), at (200) and after the position
    (201, 447: rows that have not started).  A started row's answer is the softmax over [off, pos]: counting and selection
    probes with NaN below off and above pos.  A row that has not started attends to its one current row (the hook documents:
    finite, nothing more); everything else of its cache is NaN."""
    T, H, pos = 448, 2, 200
    off = np.array([0, 57, 199, 200, 201, 73, 447], np.int32)
    started = off <= pos
    lo = np.where(started, off, pos)
    hi = np.full(len(off), pos)
    for kind in ("counting", "selection"):
        q, k, v, wants = ragged_probe(kind, T, H, lo, hi)
        r = attn(dbg, 3, q, k, v, n_keys=0, pos=pos, off=off)
        cross_plan_check(r, DAV_SELF_OFF, len(off) * H, grid_x=len(off) * H, block=256)
        for b in range(len(off)):
            got = r.out[b].reshape(H, 64)
            if not started[b]:
                assert np.isfinite(got).all(), (kind, b)
            elif kind == "counting":
                assert not A.counting_check(got, wants[b], int(hi[b] - lo[b] + 1)), (b, off[b])
            else:
                assert np.array_equal(bits(got), bits(wants[b])), (b, off[b])
    # the spread case against the f64 softmax over [off, pos]
    q, k, v = A.spread_case(len(off) * H, T, np.repeat(lo, H), np.repeat(hi, H), 5)
    r = attn(dbg, 3, *pair_major(len(off), H, q, k, v), n_keys=0, pos=pos, off=off)
    vmax = float(np.nanmax(np.abs(v)))
    for b in np.flatnonzero(started):
        for h in range(H):
            p = b * H + h
            ratio = A.spread_ratio(r.out[b, h * 64:(h + 1) * 64], A.attention_f64(q[p], k[p], v[p], int(lo[b]), int(hi[b])), vmax)
            assert ratio <= 1.0, (b, h, ratio)


def plan_of(dbg, form, B=0, C=0, N=0, H=1, T=448, n_keys=0, flags=0):
    rec = np.zeros(16, np.int32)
    rec[:13] = [form, B, C, N, H, T, n_keys, 1, 0, flags, 0, 0, 256]
    out = np.zeros(16, np.int32)
    assert dbg.lib.wmdbg_dec_attn_plan(P(rec), 1, P(out)) == 1
    return out.tolist()


@pytest.mark.parametrize("ragged", [0, 1])
def test_panels_count_every_key(dbg, ragged):
    """wmdbg_dec_self_attention_panel / _panel_off, C, w = 3, 8 with pos = 124: the rows' key counts 125 .. 132 straddle the block
    edge at 128.  The 8 rows of a window share ONE cache entry, so a row's answer is count(marked keys in its own range) / n per
    column: a key of a later position that leaked into an earlier row lights its column there."""
    C, w, H, T, pos = 3, 8, 2, 448, 124
    off = np.array([0, 5, 127], np.int32) if ragged else np.zeros(C, np.int32)
    assert plan_of(dbg, 4, C=C, N=w, H=H, T=T, flags=1 | (4 if ragged else 0))[P_VARIANT] == (DAV_SELF_OFF_PANEL if ragged else DAV_SELF_PANEL)
    rng = np.random.default_rng(9)
    q = rng.standard_normal((C * w, H * 64)).astype(np.float32)
    k = np.full((C, H, T, 64), np.nan, np.float32)
    v = np.full((C, H, T, 64), np.nan, np.float32)
    mark = np.zeros((C, H, 64), np.int64)
    for c in range(C):
        lo, last = min(int(off[c]), pos), pos + w - 1                   # (a row that has not started reads its own current row)
        k[c, :, lo:last + 1] = 0.0
        v[c, :, lo:last + 1] = 0.0
        tail = [j for j in range(pos - 2, last + 1) if j >= lo]         # the keys that tell the rows of the panel apart
        for h in range(H):
            rest = [int(x) for x in np.random.default_rng(c * 7 + h).permutation(np.arange(lo, pos - 2))]
            keys = (tail + [j for j in (lo, lo + 1, lo + 7, lo + 8, lo + 31, lo + 32, lo + 33) if j < pos - 2] + rest)[:64]
            keys = list(dict.fromkeys(keys))
            mark[c, h, :len(keys)] = keys
            mark[c, h, len(keys):] = -1
            for e, j in enumerate(keys):
                v[c, h, j, e] = 1.0
    out = np.zeros((32, H * 64), np.float32)
    if ragged:
        rc = dbg.lib.wmdbg_dec_self_attention_panel_off(dbg.handle, P(q), P(k), P(v), C, w, H, T, pos, P(off), 32, P(out))
    else:
        rc = dbg.lib.wmdbg_dec_self_attention_panel(dbg.handle, P(q), P(k), P(v), C, w, H, T, pos, 32, P(out))
    assert rc == 0, err_msg(dbg)
    assert np.all(bits(out[C * w:]) == SENT16 << 16)
    for c in range(C):
        for s in range(w):
            p = pos + s
            lo = min(int(off[c]), p)
            n = p - lo + 1
            got = out[c * w + s].reshape(H, 64)
            if p < off[c]:                  # not started: finite, nothing more
                assert np.isfinite(got).all(), (c, s)
                continue
            m = np.where((mark[c] >= lo) & (mark[c] <= p), mark[c], -1)
            bad = A.counting_check(got, m, n)
            assert not bad, (c, s, n, bad[:6])


# ------------------------------------------------------------------ live lists
LIVE_LISTS = [[0, 2, 3, 5], [0, 1, 2], [4]]      # thinned; an empty tail (rows 3 .. 5 have left); one live row


def live_case(dbg, form, rows, H, T, n, make):
    """make(k, v, live) -> the launch result.  Live rows have the bits of the all-live launch although the caches of the rows
    that left are NaN; rows that are not live hold the sentinel."""
    q, k, v = A.spread_case(rows * H, T, 0, n - 1, 21 + form)
    q, k, v = pair_major(rows, H, q, k, v)
    full = make(q, k, v, None)
    assert np.isfinite(full.out).all()
    for live in LIVE_LISTS + [list(range(rows))]:
        dead = [b for b in range(rows) if b not in live]
        kd, vd = k.copy(), v.copy()
        kd[dead], vd[dead] = np.nan, np.nan
        r = make(q, kd, vd, live)
        assert np.array_equal(bits(r.out[live]), bits(full.out[live])), (form, live)
        assert np.all(bits(r.out[dead]) == SENT16 << 16) and np.all(bits(r.pad) == SENT16 << 16), (form, live)
    return full


def test_live_lists_cross_and_self(dbg):
    live_case(dbg, 0, 6, 2, 1500, 437, lambda q, k, v, live: attn(dbg, 0, q, k, v, n_keys=437, live=live))
    with tuning(dbg, xattn_wgs=4):          # the persistent walk over a thinned list: 12 pairs on 4 workgroups
        live_case(dbg, 0, 6, 2, 1500, 437, lambda q, k, v, live: attn(dbg, 0, q, k, v, n_keys=437, live=live))
    live_case(dbg, 3, 6, 2, 448, 130, lambda q, k, v, live: attn(dbg, 3, q, k, v, n_keys=130, live=live))
    live_case(dbg, 3, 6, 2, 448, 130, lambda q, k, v, live: attn(dbg, 3, q, k, v, n_keys=0, pos=129, live=live))


# ------------------------------------------------------------------ the fused query (form 2)
def fq_side(B, K, seed):
    """the query side: x [B][K] with a common-mode offset, LayerNorm weights, Wq with std 3 / sqrt(K) (scores of standard
    deviation ~3 once scaled by 1 / 8 and multiplied with unit keys), a bias"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, K)) * 2 * (1 + 0.5 * np.arange(B) / B)[:, None] + 0.3).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    Wq = A.bf16(rng.standard_normal((K, K)) * 3.0 / np.sqrt(K) + np.linspace(-0.02, 0.02, K)[:, None])
    bias = rng.standard_normal(K).astype(np.float32)
    return x, g, beta, Wq, bias


def layer_norm64(x, g, b):
    x = x.astype(np.float64)
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def gemv_q(dbg, side):
    """the product's first launch when it does not fuse: wmdbg_dec_gemv_ln, DE_Q, centre = 1 -> (q f32 [B][K], mean [B])"""
    x, g, beta, Wq, bias = side
    B, K = x.shape
    o = np.zeros((B, K), np.float32)
    mean, Wf, c1, c2 = np.zeros(B, np.float32), np.zeros((K, K), np.float32), np.zeros(K, np.float32), np.zeros(K, np.float32)
    rc = dbg.lib.wmdbg_dec_gemv_ln(dbg.handle, DE_Q, P(x), P(g), P(beta), P(Wq), P(bias), B, K, K, 1, 0, 0, 0, P(o), None, None, None,
                                   P(mean), P(Wf), P(c1), P(c2))
    assert rc == 0, err_msg(dbg)
    return o, mean


FQ_CASES = [(16, 6, 384, 2, 6), (8, 12, 768, 4, 6), (6, 16, 1024, 4, 8), (6, 18, 1152, 6, 6), (5, 20, 1280, 5, 8), (24, 8, 512, 2, 8)]


@pytest.mark.parametrize("B,H,K,spw,nw", FQ_CASES)
def test_fused_query(dbg, B, H, K, spw, nw):
    """dec_xattn_fq_kernel, one case per instantiation and K split, T = n_keys = 600 (two full blocks and a tail of 88).
    (a) bit for bit the two launches the product would otherwise make: wmdbg_dec_gemv_ln (DE_Q, centre = 1), then form 0 with
        nsplit = 1 on that query; mean_out equal to the GEMV's.
    (b) against f64 -- LayerNorm, projection (on the bf16 activations the kernel multiplies), attention -- with the per-element
        gate of the spread case plus the LN-GEMV tolerance of test_decode_step_kernels_gpu.py CARRIED through the scores: a
        query element is within eq = 4e-3 max|q_ref|, so a score moves by at most D = eq * max_j sum_e |k[j][e]| / 8, every
        softmax weight by a factor within e^(+-2 D), and the output by at most (e^(2 D) - 1) max|v| (sum_j |w'_j - w_j| <= e^(2 D) - 1).
    (c) against f64 attention over the GPU's own query of (a): the plain spread gate, nothing carried.
    (d) the counting probe (k = 0: exact whatever the query).
    The 24-row case has two 16-row blocks: rows 16 .. 23 are asserted on their own."""
    T = n = 600
    side = fq_side(B, K, 100 + K)
    q, k, v = A.spread_case(B * H, T, 0, n - 1, K)
    _, k, v = pair_major(B, H, q, k, v)
    r = attn(dbg, 2, None, k, v, n_keys=n, fq=side)
    assert r.plan[P_STATUS] == 0 and r.plan[P_VARIANT] == DAV_FQ and r.plan[P_SPW] == spw, r.plan
    assert r.plan[P_LDS] == (nw * 1024 + 192) * 4 and r.plan[P_BLOCK] == 512 and r.plan[P_NWG] == 8 * -(-B * H // 8), r.plan
    assert r.plan[P_RULE] == 1, "wm_dec_xattn_fq_applies does not hold for the shape"
    assert np.all(bits(r.pad) == SENT16 << 16)
    # (a)
    q_gpu, mean_gpu = gemv_q(dbg, side)
    two = attn(dbg, 0, q_gpu, k, v, n_keys=n, nsplit=1)
    cross_plan_check(two, DAV_STREAM, B * H)
    assert np.array_equal(bits(r.out), bits(two.out))
    assert np.array_equal(bits(r.mean), bits(mean_gpu))
    if B > 16:
        assert np.array_equal(bits(r.out[16:]), bits(two.out[16:])) and np.isfinite(r.out[16:]).all()
    # (b), (c)
    x, g, beta, Wq, bias = side
    q_ref = A.bf16(layer_norm64(x, g, beta)).astype(np.float64) @ Wq.astype(np.float64).T + bias
    eq = 4e-3 * np.abs(q_ref).max()
    assert np.abs(q_gpu - q_ref).max() <= eq
    vmax = float(np.nanmax(np.abs(v)))
    D = eq * np.abs(k[:, :, :n]).sum(-1).max() / 8.0
    ref_b = A.attention_rows(q_ref.astype(np.float32), k, v, 0, n - 1)
    ref_c = A.attention_rows(q_gpu, k, v, 0, n - 1)
    rb = A.spread_ratio(r.out, ref_b, vmax, extra=np.expm1(2 * D) * vmax)
    rc = A.spread_ratio(r.out, ref_c, vmax)
    print("fused query B %d H %d K %d: carried score bound D = %.3f; |out - f64| at %.3f of the carried gate, at %.3f of the plain "
          "gate against the f64 attention over the GPU's query" % (B, H, K, D, rb, rc))
    assert rb <= 1.0 and rc <= 1.0
    if B > 16:
        assert A.spread_ratio(r.out[16:], ref_c[16:], vmax) <= 1.0
    # (d)
    qc, kc, vc, marks = A.counting_probe(B * H, T, 0, n - 1, A.NS_CROSS)
    _, kc, vc = pair_major(B, H, qc, kc, vc)
    rc_ = attn(dbg, 2, None, kc, vc, n_keys=n, fq=side)
    bad = A.counting_check(rc_.out.reshape(B * H, 64), marks, n)
    assert not bad, bad[:8]


def test_live_lists_fused_query(dbg):
    B, H, K, T, n = 16, 6, 384, 600, 437
    side = fq_side(B, K, 7)
    live_lists = [[0, 2, 3, 5, 9, 15], [0, 1, 2], [4]]
    q, k, v = A.spread_case(B * H, T, 0, n - 1, 31)
    _, k, v = pair_major(B, H, q, k, v)
    full = attn(dbg, 2, None, k, v, n_keys=n, fq=side)
    assert full.plan[P_VARIANT] == DAV_FQ and np.isfinite(full.out).all()
    for live in live_lists:
        dead = [b for b in range(B) if b not in live]
        kd, vd = k.copy(), v.copy()
        kd[dead], vd[dead] = np.nan, np.nan
        r = attn(dbg, 2, None, kd, vd, n_keys=n, fq=side, live=live)
        assert np.array_equal(bits(r.out[live]), bits(full.out[live])), live
        assert np.array_equal(bits(r.mean[live]), bits(full.mean[live])), live
        assert np.all(bits(r.out[dead]) == SENT16 << 16), live


# ------------------------------------------------------------------ warm-up workgroups
def test_warm_up_workgroups_change_no_bit(dbg):
    """B <= 16, compute workgroups a multiple of 8, a 64 x 128 matrix behind them: the plan reports 4 warm-up tiles and the grid
    grows by them; outputs as without the matrix -- stream, self and fused query."""
    q, k, v = A.spread_case(8, 1500, 0, 436, 41)
    qkv = pair_major(4, 2, q, k, v)
    cases = [("stream", lambda w: attn(dbg, 0, *qkv, n_keys=437, warm=w), DAV_STREAM, 8)]
    q3, k3, v3 = A.spread_case(8, 448, 0, 129, 42)
    qkv3 = pair_major(4, 2, q3, k3, v3)
    cases.append(("self", lambda w: attn(dbg, 3, *qkv3, n_keys=0, pos=129, warm=w), DAV_SELF, 8))
    side = fq_side(16, 384, 43)
    q2, k2, v2 = A.spread_case(96, 600, 0, 599, 44)
    _, k2, v2 = pair_major(16, 6, q2, k2, v2)
    cases.append(("fused query", lambda w: attn(dbg, 2, None, k2, v2, n_keys=600, fq=side, warm=w), DAV_FQ, 96))
    for what, run, variant, n_wg in cases:
        plain, warm = run((0, 0)), run((64, 128))
        assert plain.plan[P_VARIANT] == warm.plan[P_VARIANT] == variant, what
        assert plain.plan[P_WARM] == 0 and plain.plan[P_GRID_X] == n_wg, (what, plain.plan)
        assert warm.plan[P_WARM] == 4 and warm.plan[P_NWG] == n_wg and warm.plan[P_GRID_X] == n_wg + 4, (what, warm.plan)
        assert warm.plan[P_TILE_BYTES] == 16 * 128 * 2
        assert np.isfinite(plain.out).all() and np.array_equal(bits(plain.out), bits(warm.out)), what
        assert np.array_equal(bits(plain.mean), bits(warm.mean)), what
    odd = attn(dbg, 0, *pair_major(3, 2, q[:6], k[:6], v[:6]), n_keys=437, warm=(64, 128))     # 6 workgroups: no multiple of 8, no warm-up
    assert odd.plan[P_WARM] == 0 and odd.plan[P_GRID_X] == 6


# ------------------------------------------------------------------ candidate groups
@pytest.mark.parametrize("C,N,H,T,variant", [(1, 5, 6, 1500, DAV_CAND_FLAT), (13, 3, 20, 600, DAV_CAND)])
def test_candidate_groups(dbg, C, N, H, T, variant):
    """dec_xcand_attn_kernel through the existing hooks (plain and _shared) and through form 1 (whose plan record is asserted):
    the N candidates of a window read ONE cache.  Counting: every candidate of a pair gets the pair's counts.  Selection: the
    candidates of a pair select DIFFERENT keys of the shared cache."""
    n = T - 63
    pairs = C * H
    rows = C * N
    # counting
    qc, k, v, marks = A.counting_probe(pairs, T, 0, n - 1, A.NS_CROSS)
    k, v = A.heads(k, C, H), A.heads(v, C, H)
    q = np.random.default_rng(C).standard_normal((rows, H * 64)).astype(np.float32)
    runs = []

    def launch_all(q, k, v):
        r = attn(dbg, 1, q, k, v, n_keys=n, N=N)
        assert r.plan[P_STATUS] == 0 and r.plan[P_VARIANT] == variant, r.plan
        assert (r.plan[P_COMBINE] == rows * H) == (variant == DAV_CAND_FLAT)
        if variant == DAV_CAND:
            assert r.plan[P_NWG] == 130 and r.plan[P_BLOCK] == 512         # 260 pairs: two rounds, balanced
        assert np.all(bits(r.pad) == SENT16 << 16)
        outs = [r.out]
        for fn in (dbg.lib.wmdbg_dec_attention_cand, dbg.lib.wmdbg_dec_attention_cand_shared):
            o = np.zeros((rows, H * 64), np.float32)
            assert fn(dbg.handle, P(q), P(k), P(v), C, N, H, T, n, None, rows, P(o)) == 0, err_msg(dbg)
            outs.append(o)
        sh = attn(dbg, 1, q, k, v, n_keys=n, N=N, short=1)
        assert sh.plan[P_VARIANT] == DAV_CAND and sh.plan[P_NWG] == pairs and sh.plan[P_COMBINE] == 0, sh.plan
        outs.append(sh.out)
        return outs

    for o in launch_all(q, k, v):
        o = o.reshape(C, N, H, 64)
        for s in range(N):
            bad = A.counting_check(o[:, s].reshape(pairs, 64), marks, n)
            assert not bad, (s, bad[:6])
    # selection: candidate s of pair p selects key sel[p * N + s]
    sel = selection_keys(n, A.NS_CROSS, pairs * N)
    _, k, v, _ = A.selection_probe(CODE, [0] * pairs, T, 0, n - 1)
    want = np.stack([v[p, sel[p * N + s]] for p in range(pairs) for s in range(N)]).reshape(C, H, N, 64)
    q = np.stack([CODE[sel[p * N + s]] for p in range(pairs) for s in range(N)]).reshape(C, H, N, 64)
    q = np.ascontiguousarray(q.transpose(0, 2, 1, 3)).reshape(rows, H * 64)
    want = np.ascontiguousarray(want.transpose(0, 2, 1, 3)).reshape(rows, H * 64)
    for o in launch_all(q, A.heads(k, C, H), A.heads(v, C, H)):
        assert np.array_equal(bits(o), bits(want))


# ------------------------------------------------------------------ the spread numeric case, one shape of every variant
def test_spread_case_every_variant(dbg):
    """Per-element gate |out - ref| <= 2^-8 |ref| + 2^-12 max|v| against the f64 softmax, at one shape of every launch variant.
    The measured figures are in the module docstring; launches of the same pairs print the same figure whatever the variant,
    because the bits are the same."""
    worst = {}
    for name, (B, H, T, nsplit, knobs, short, variant, want) in CROSS.items():
        if name.endswith(("40_pairs", "65_pairs")) and "stream" not in name:
            continue
        n = T - 63 if T > 100 else T
        q, k, v = A.spread_case(B * H, T, 0, n - 1, 61)
        vmax = float(np.nanmax(np.abs(v)))
        with tuning(dbg, **knobs):
            r = attn(dbg, 0, *pair_major(B, H, q, k, v), n_keys=n, nsplit=nsplit, short=short)
        cross_plan_check(r, variant, B * H)
        ref = np.stack([A.attention_f64(q[p], k[p], v[p], 0, n - 1) for p in range(B * H)]).reshape(B, H * 64)
        worst[name] = A.spread_ratio(r.out, ref, vmax)
    q, k, v = A.spread_case(8, 448, 0, 299, 62)
    vmax = float(np.nanmax(np.abs(v)))
    ref = np.stack([A.attention_f64(q[p], k[p], v[p], 0, 299) for p in range(8)]).reshape(4, 128)
    for name, kw in (("self_const", dict(n_keys=300)), ("self_device_pos", dict(n_keys=0, pos=299))):
        r = attn(dbg, 3, *pair_major(4, 2, q, k, v), **kw)
        assert r.plan[P_VARIANT] == DAV_SELF
        worst[name] = A.spread_ratio(r.out, ref, vmax)
    # candidate groups: N = 3 candidates of 2 windows x 3 heads share the caches
    C, N, H, T, n = 2, 3, 3, 1500, 1437
    q, k, v = A.spread_case(C * H, T, 0, n - 1, 63)
    vmax = float(np.nanmax(np.abs(v)))
    qs = (3.0 * np.random.default_rng(64).standard_normal((C * N, H * 64))).astype(np.float32)
    kk, vv = A.heads(k, C, H), A.heads(v, C, H)
    ref = A.attention_rows(qs, kk, vv, 0, n - 1, entry=[r // N for r in range(C * N)])
    for name, short, variant in (("cand_flat", 0, DAV_CAND_FLAT), ("cand_short_lived", 1, DAV_CAND)):
        r = attn(dbg, 1, qs, kk, vv, n_keys=n, N=N, short=short)
        assert r.plan[P_VARIANT] == variant
        worst[name] = A.spread_ratio(r.out, ref, vmax)
    for name, ratio in worst.items():
        print("spread case %-28s worst |out - ref| / gate = %.3f" % (name, ratio))
    assert all(ratio <= 1.0 for ratio in worst.values()), worst


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_sentinel(dbg):
    def refused(r, word):
        assert r.rc == WM_ERR_INVALID and word in err_msg(dbg), (r.rc, err_msg(dbg))
        assert np.all(bits(r.full) == SENT16 << 16), "a refused call wrote its output"

    q = np.zeros((2, 64), np.float32)
    big = np.zeros((2, 1, 1537, 64), np.float32)
    r = attn(dbg, 0, q, big, big, n_keys=8, expect_ok=False)                                       # T > 1536
    refused(r, "1536")
    assert r.plan[P_STATUS] == WM_ERR_INVALID
    r = attn(dbg, 3, q, big, big, n_keys=8, expect_ok=False)
    refused(r, "1536")
    kv = np.zeros((2, 1, 64, 64), np.float32)
    wide_q, wide = np.zeros((1, 256 * 64), np.float32), np.zeros((1, 256, 8, 64), np.float32)
    refused(attn(dbg, 0, wide_q, wide, wide, n_keys=8, nsplit=2, expect_ok=False), "packed")       # H = 256 overflows packA's 8 bits
    refused(attn(dbg, 0, q, kv, kv, n_keys=8, nsplit=3, expect_ok=False), "nsplit")
    refused(attn(dbg, 0, q, kv, kv, n_keys=65, expect_ok=False), "keys")                            # more keys than cache rows
    refused(attn(dbg, 0, q, kv, kv, n_keys=0, expect_ok=False), "keys")
    refused(attn(dbg, 3, q, kv, kv, pos=64, expect_ok=False), "keys")                               # position behind the cache
    for bad in ([0, 64], [-1, 0]):
        refused(attn(dbg, 3, q, kv, kv, pos=10, off=bad, expect_ok=False), "off[")                  # off out of range
    refused(attn(dbg, 0, q, kv, kv, n_keys=8, live=[1, 0], expect_ok=False), "ascending")           # not ascending
    refused(attn(dbg, 0, q, kv, kv, n_keys=8, live=[0, 2], expect_ok=False), "ascending")           # not a row of the group
    r = attn(dbg, 1, np.zeros((9, 64), np.float32), kv[:1], kv[:1], n_keys=8, N=9, expect_ok=False)     # (no row count to fill by)
    assert r.rc == WM_ERR_INVALID and "candidates" in err_msg(dbg)
    ok = attn(dbg, 0, q, kv, kv, n_keys=8)                                                          # ... and the hook still works
    assert ok.rc == 0 and np.array_equal(ok.out, np.zeros((2, 64), np.float32))


# ------------------------------------------------------------------ encoder attention, the same probes
@pytest.mark.parametrize("mfma_sum", [0, 1])
@pytest.mark.parametrize("S", [64, 129, 200, 1500])
def test_encoder_attention_exact(dbg, S, mfma_sum):
    """wmdbg_enc_attention (enc_attn_kernel, both row-sum variants).  Selection: query i selects key pi(i) of a fixed
    permutation, so one launch covers every (query, key) pair once and the output row is v[pi(i)] bit for bit -- which also
    pins wm_att_vt_pos and the pad columns behind S.  The kernel's query is pre-scaled by 0.125 log2(e) and rounded to bf16
    (a score moves by at most 0.25 in natural units), against a lead of 56.  Counting: q = 0, so every key weighs 1 / S."""
    H = 2
    d = H * 64
    perm = np.random.default_rng(S).permutation(S)
    k = np.zeros((1, S, d), np.float32)
    v = np.zeros((1, S, d), np.float32)
    q = np.zeros((1, S, d), np.float32)
    for h in range(H):
        pi = np.roll(perm, 17 * h)
        k[0, :, h * 64:(h + 1) * 64] = 16.0 * CODE[:S]
        v[0, :, h * 64:(h + 1) * 64] = A.probe_values(h, S)
        q[0, :, h * 64:(h + 1) * 64] = CODE[pi]
    want = np.concatenate([A.probe_values(h, S)[np.roll(perm, 17 * h)] for h in range(H)], axis=1)
    with tuning(dbg, enc_attn_mfma_sum=mfma_sum):
        out = np.zeros((1, S, d), np.float32)
        assert dbg.lib.wmdbg_enc_attention(dbg.handle, P(q), P(k), P(v), 1, H, S, P(out)) == 0, err_msg(dbg)
        miss = np.flatnonzero((bits(out[0]) != bits(want)).any(axis=1))
        assert miss.size == 0, ("selection: query rows whose output is not v[pi(i)]", miss[:10], perm[miss[:10]])
        # counting: column (h, e) marks key (h * 64 + e) * step (every key when S <= H * 64)
        Hc = -(-S // 64)
        dc = Hc * 64
        vc = np.zeros((1, S, dc), np.float32)
        vc[0, np.arange(S), np.arange(S)] = 1.0
        zero = np.zeros((1, S, dc), np.float32)
        out = np.zeros((1, S, dc), np.float32)
        assert dbg.lib.wmdbg_enc_attention(dbg.handle, P(zero), P(zero), P(vc), 1, Hc, S, P(out)) == 0, err_msg(dbg)
    marked = np.abs(out[0, :, :S] - 1.0 / S) <= A.bf16_ulp(1.0 / S)
    assert marked.all(), ("counting: (query, key) pairs not counted once", np.argwhere(~marked)[:8], out[0, :, :S][~marked][:8], 1.0 / S)
    assert np.all(out[0, :, S:] == 0.0)
