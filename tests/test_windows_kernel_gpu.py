"""Kernel-level GPU tests of the window-set copy (csrc/xkv_rows.hip) through wmdbg_xkv_rows: whole windows between a decode
group's cross-K/V cache [2L][cap_b][H][1500][64] and a set's window-major store [W][2L][H][1500][64], in both directions.
Every comparison is exact (array_equal) against numpy fancy indexing on random bf16 bit patterns."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, H, W = 2, 2, 5
L2 = 2 * L
SLAB = H * 1500 * 64          # elements of one (layer, k|v) slab of a window
CANARY = 0xBEEF


@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_xkv_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.wmdbg_xkv_rows.restype = ctypes.c_int
    ctx = pkg.binding.Context(debug=True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def store_bits():
    """The reference store, computed once and never written: [W][2L][SLAB] random bf16 bit patterns."""
    a = np.random.default_rng(31).integers(0, 1 << 16, size=(W, L2, SLAB), dtype=np.uint16)
    a.setflags(write=False)
    return a


def _copy(ctx, d_group, cap, d_store, store_rows, rows, to_store):
    r = np.ascontiguousarray(rows, dtype=np.int32)
    st = ctx.lib.wmdbg_xkv_rows(ctx.handle, d_group, cap, d_store, store_rows, r.ctypes.data_as(ctypes.c_void_p), r.size, L, H,
                                1 if to_store else 0)
    assert st == 0, ctx.lib.wm_last_error()


MAPS = [(3, [0]), (3, [4, 0, 2]), (17, [0]), (17, [4, 0, 2]), (17, [3, 3, 1, 3]), (17, [2, 4, 0, 3, 1])]


@pytest.mark.parametrize("cap,rows", MAPS)
def test_gather_equals_fancy_indexing_and_leaves_the_other_rows_alone(dbg, store_bits, cap, rows):
    d_store = dbg.to_device(store_bits)
    d_group = dbg.to_device(np.full((L2, cap, SLAB), CANARY, dtype=np.uint16))
    try:
        _copy(dbg, d_group, cap, d_store, W, rows, False)
        got = dbg.download(d_group, (L2, cap, SLAB), np.uint16)
        assert np.array_equal(dbg.download(d_store, store_bits.shape, np.uint16), store_bits)   # the source is read only
    finally:
        dbg.dev_free(d_group)
        dbg.dev_free(d_store)
    n = len(rows)
    assert np.array_equal(got[:, :n], store_bits[rows].transpose(1, 0, 2))
    assert np.all(got[:, n:] == CANARY)


@pytest.mark.parametrize("cap,rows", [m for m in MAPS if len(set(m[1])) == len(m[1])])
def test_scatter_equals_fancy_indexing_and_gather_after_scatter_is_the_identity(dbg, cap, rows):
    rng = np.random.default_rng(cap * 100 + len(rows))
    group = rng.integers(0, 1 << 16, size=(L2, cap, SLAB), dtype=np.uint16)
    d_group = dbg.to_device(group)
    d_store = dbg.to_device(np.full((W, L2, SLAB), CANARY, dtype=np.uint16))
    d_back = dbg.to_device(np.full((L2, cap, SLAB), CANARY, dtype=np.uint16))
    try:
        _copy(dbg, d_group, cap, d_store, W, rows, True)
        store = dbg.download(d_store, (W, L2, SLAB), np.uint16)
        _copy(dbg, d_back, cap, d_store, W, rows, False)
        back = dbg.download(d_back, (L2, cap, SLAB), np.uint16)
    finally:
        for p in (d_group, d_store, d_back):
            dbg.dev_free(p)
    n = len(rows)
    want = np.full((W, L2, SLAB), CANARY, dtype=np.uint16)
    want[rows] = group[:, :n].transpose(1, 0, 2)
    assert np.array_equal(store, want)                       # the rows named, and only those
    assert np.array_equal(back[:, :n], group[:, :n]) and np.all(back[:, n:] == CANARY)


def test_bad_row_maps_are_rejected(dbg):
    d = dbg.dev_malloc(L2 * 3 * SLAB * 2)
    try:
        r = np.array([5], np.int32)
        p = r.ctypes.data_as(ctypes.c_void_p)
        assert dbg.lib.wmdbg_xkv_rows(dbg.handle, d, 3, d, W, p, 1, L, H, 0) == 1            # a row past the store
        assert dbg.lib.wmdbg_xkv_rows(dbg.handle, d, 3, d, W, p, 4, L, H, 0) == 1            # more rows than the group holds
        r2 = np.array([1, 1], np.int32)
        assert dbg.lib.wmdbg_xkv_rows(dbg.handle, d, 3, d, W, r2.ctypes.data_as(ctypes.c_void_p), 2, L, H, 1) == 1   # scatter twice
    finally:
        dbg.dev_free(d)


def test_store_rows_beyond_4_gib_use_64_bit_offsets(dbg, pkg):
    """A store row that starts past byte 2^32 (and so past element 2^31): a sparse 4.3 GB allocation of which only the slabs
    used are ever touched.  Rows 0 .. 4 hold canaries: offsets truncated to 32 bits would land in row 3."""
    row_bytes = L2 * SLAB * 2
    far = (1 << 32) // row_bytes + 4                       # 2800
    assert far * row_bytes > 1 << 32 and far * L2 * SLAB > 1 << 31
    assert (far * row_bytes) % (1 << 32) // row_bytes < 5
    n_rows = far + 1
    lib = dbg.lib
    rng = np.random.default_rng(77)
    far_bits = rng.integers(0, 1 << 16, size=(L2, SLAB), dtype=np.uint16)
    near_bits = rng.integers(0, 1 << 16, size=(L2, SLAB), dtype=np.uint16)
    low = np.full((5, L2, SLAB), CANARY, dtype=np.uint16)
    low[1] = near_bits
    d_store = dbg.dev_malloc(n_rows * row_bytes)
    at = lambda row: ctypes.c_void_p(d_store.value + row * row_bytes)
    d_group = dbg.to_device(np.full((L2, 3, SLAB), CANARY, dtype=np.uint16))
    try:
        dbg.upload(d_store, low)
        dbg.upload(at(far), far_bits)
        _copy(dbg, d_group, 3, d_store, n_rows, [far, 1], False)
        got = dbg.download(d_group, (L2, 3, SLAB), np.uint16)
        assert np.array_equal(got[:, 0], far_bits) and np.array_equal(got[:, 1], near_bits) and np.all(got[:, 2] == CANARY)
        # and the other way: group rows 0, 1 (far, near) -> store rows 1, far: the two exchange places
        _copy(dbg, d_group, 3, d_store, n_rows, [1, far], True)
        assert np.array_equal(dbg.download(at(far), (L2, SLAB), np.uint16), near_bits)
        low_after = dbg.download(d_store, (5, L2, SLAB), np.uint16)
        assert np.array_equal(low_after[1], far_bits)
        assert np.all(low_after[[0, 2, 3, 4]] == CANARY)
    finally:
        dbg.dev_free(d_group)
        dbg.dev_free(d_store)
    assert lib.wm_last_error() is not None
