"""The two launches a prompt panel of a RAGGED decode group adds (wm_set_prompt_panel), one by one through the debug library's
hooks: the panel self-attention with the windows' offsets against the step path's ragged launch, position by position, and
the panel embedding with offsets against the step path's embeddings, row by row.  Raw bits throughout: a panel changes which
rows share a launch, never a row's arithmetic.  Geometry: tiny.en (d 384, 6 heads, 448 positions)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, D, H = 448, 384, 6
SENT16 = np.uint32(0x7fc50000)   # WMDBG_SENTINEL_BF16 widened to f32
KINDS = ("zero", "before", "inside", "last", "beyond")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf(a):
    """f32 values that are exact in bf16 (round to nearest even)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    vp, ip = ctypes.c_void_p, ctypes.c_int
    lib = c.lib
    lib.wmdbg_dec_self_attention_off.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, vp, vp]
    lib.wmdbg_dec_self_attention_panel_off.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    lib.wmdbg_dec_embed_panel_off.argtypes = [vp, vp, vp, ip, ip, ip, vp] + [ip] * 5 + [vp, ip] + [vp] * 4
    yield c
    c.close()


def ok(dbg, st):
    assert st == 0, dbg.lib.wm_last_error()


# ---------------------------------------------------------------- 1. self-attention
def _positions(w):
    """panel starts whose rows' key counts (offset 0: p + 1) cross 8, 32 and 127 / 128 / 129, and the panel that ends the cache"""
    def cross(n):   # counts n and n + 1 (w = 2), n - 1 .. n + 1 (w = 3), n - 3 .. n + 4 (w = 8)
        return n - 1 - (w - 1) // 2
    pos = [cross(8), cross(32), cross(128), T - w]
    if w == 2:
        pos.insert(2, 126)   # counts 127, 128 (cross(128) gives 128, 129)
    return pos


def _offset(kind, pos, w, rng):
    if kind == "zero":
        return 0
    if kind == "before":     # < pos: every row of the panel has started; the relative key counts differ from p + 1
        return int(rng.integers(1, pos)) if pos > 1 else 0
    if kind == "inside":     # pos < off <= pos + w - 1: the window starts in the middle of the panel
        return int(rng.integers(pos + 1, pos + w)) if w > 1 else pos
    if kind == "last":       # the window's first token is the panel's last row
        return pos + w - 1
    return int(rng.integers(pos + w, T))   # beyond the panel: no row has started


@pytest.mark.parametrize("w", [2, 3, 8])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_ragged_panel_rows_are_the_step_kernels_rows(dbg, C, w):
    rng = np.random.default_rng(1000 * C + w)
    k = bf(rng.standard_normal((C, H, T, 64)))
    v = bf(rng.standard_normal((C, H, T, 64)) + np.linspace(-1, 1, 64))
    nan = np.float32(np.nan)
    seen = set()
    for pi, pos in enumerate(_positions(w)):
        kinds = [kd for kd in KINDS if kd != "beyond" or pos + w < T]
        # one window: every kind in turn; more: the kinds dealt over the windows, rotated from one position to the next
        rounds = [[kd] for kd in kinds] if C == 1 else [[kinds[(c + pi) % len(kinds)] for c in range(C)]]
        for kd_row in rounds:
            seen.update(kd_row)
            off = np.array([_offset(kd, pos, w, rng) for kd in kd_row], dtype=np.int32)
            q = rng.standard_normal((C * w, H * 64)).astype(np.float32)
            kk, vv = k.copy(), v.copy()
            for c in range(C):
                first = min(int(off[c]), pos)    # in front of every row's keys: NaN bit patterns that must reach no output
                kk[c, :, :first] = nan
                vv[c, :, :first] = nan
            kk[:, :, pos + w:] = nan             # behind the panel: what no step has appended yet
            vv[:, :, pos + w:] = nan
            rows = ((C * w + 15) // 16) * 16 + 16
            out = np.zeros((rows, H * 64), np.float32)
            ok(dbg, dbg.lib.wmdbg_dec_self_attention_panel_off(dbg.handle, P(q), P(kk), P(vv), C, w, H, T, pos, P(off), rows, P(out)))
            assert np.all(bits(out[C * w:]) == SENT16), (w, pos)
            assert np.isfinite(out[:C * w]).all(), (w, pos, off.tolist())   # rows that have not started included
            for s in range(w):
                p = pos + s
                k1, v1 = kk.copy(), vv.copy()
                k1[:, :, p + 1:] = nan           # the step at position p has appended nothing behind p
                v1[:, :, p + 1:] = nan
                for c in range(C):               # ... and needs nothing in front of the row's own first key
                    k1[c, :, :min(int(off[c]), p)] = nan
                    v1[c, :, :min(int(off[c]), p)] = nan
                want = np.full((C, H * 64), np.nan, np.float32)
                ok(dbg, dbg.lib.wmdbg_dec_self_attention_off(dbg.handle, P(np.ascontiguousarray(q[s::w])), P(k1), P(v1), C, H, T, p,
                                                             P(off), P(want)))
                started = off <= p
                got = out[s:C * w:w]
                assert np.array_equal(bits(got[started]), bits(want[started])), (w, pos, s, off.tolist())
    assert seen == set(KINDS)


def test_ragged_panel_with_offsets_zero_is_the_uniform_panel(dbg):
    vp, ip = ctypes.c_void_p, ctypes.c_int
    dbg.lib.wmdbg_dec_self_attention_panel.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    C, w, pos = 5, 8, 124
    rng = np.random.default_rng(7)
    k = bf(rng.standard_normal((C, H, T, 64)))
    v = bf(rng.standard_normal((C, H, T, 64)))
    q = rng.standard_normal((C * w, H * 64)).astype(np.float32)
    a, b = np.zeros((48, H * 64), np.float32), np.zeros((48, H * 64), np.float32)
    ok(dbg, dbg.lib.wmdbg_dec_self_attention_panel_off(dbg.handle, P(q), P(k), P(v), C, w, H, T, pos, P(np.zeros(C, np.int32)), 48, P(a)))
    ok(dbg, dbg.lib.wmdbg_dec_self_attention_panel(dbg.handle, P(q), P(k), P(v), C, w, H, T, pos, 48, P(b)))
    assert np.array_equal(bits(a), bits(b))


def test_ragged_panel_rejects_bad_geometry(dbg):
    z = np.zeros(1 << 16, np.float32)
    good = np.zeros(17, np.int32)
    for C, w, pos, off in ((1, 9, 0, good), (17, 8, 0, good), (1, 8, T - 7, good), (2, 2, 0, np.array([0, T], np.int32)),
                           (2, 2, 0, np.array([-1, 0], np.int32))):
        assert dbg.lib.wmdbg_dec_self_attention_panel_off(dbg.handle, P(z), P(z), P(z), C, w, 1, T, pos, P(off), 144, P(z)) == 1
    assert dbg.lib.wmdbg_dec_self_attention_panel_off(dbg.handle, P(z), P(z), P(z), 1, 2, 1, T, 0, None, 144, P(z)) == 1


# ---------------------------------------------------------------- 2. embedding
@pytest.mark.parametrize("stride,c0,C,w,pos", [(5, 1, 4, 8, 0), (17, 12, 5, 5, 443), (16, 0, 16, 8, 8), (4, 0, 4, 1, 0),
                                                (4, 0, 4, 1, 17), (20, 3, 17, 7, 1), (6, 1, 5, 3, 30)])
def test_ragged_embed_panel_equals_the_step_paths_embeddings(dbg, stride, c0, C, w, pos):
    rng = np.random.default_rng(stride * 100 + w + pos)
    V, n_ctx = 1000, T
    emb = bf(rng.standard_normal((V, D)) * 0.1)
    pemb = (rng.standard_normal((n_ctx, D)) * 0.1 + 0.5).astype(np.float32)
    seq = rng.integers(0, V, size=(n_ctx, stride)).astype(np.int32)
    # offsets: 0, in front of the panel, inside it (a row that starts mid-panel), its last row, behind it (not started)
    cand = [0, pos // 2, pos + w // 2, pos + w - 1, min(pos + w + 3, n_ctx - 1)]
    off = np.array([cand[c % len(cand)] for c in range(C)], dtype=np.int32)
    got = []
    for by_steps in (0, 1):
        x = np.zeros((C * w, D), np.float32)
        xb = np.zeros((C * w, D), np.float32)
        st = np.zeros((C * w, D // 16, 2), np.float32)
        mean = np.zeros(C * w, np.float32)
        ok(dbg, dbg.lib.wmdbg_dec_embed_panel_off(dbg.handle, P(emb), P(pemb), V, D, n_ctx, P(seq), stride, c0, C, w, pos, P(off),
                                                  by_steps, P(x), P(xb), P(st), P(mean)))
        got.append((x, xb, st, mean))
    for a, b_, name in zip(got[0], got[1], ("x", "xb", "stats", "mean")):
        assert np.array_equal(bits(a), bits(b_)), name
    x, xb, st, mean = got[0]
    for c in range(C):     # ... and they are the rows asked for: the positional row counts from the window's offset
        for s in range(w):
            want = emb[seq[pos + s, c0 + c]] + pemb[max(pos + s - int(off[c]), 0)]
            assert np.array_equal(x[c * w + s], want), (c, s)
    assert np.all(st[:, 1:] == 0) and np.all(np.isfinite(st)) and np.all(np.isfinite(xb)) and np.all(np.isfinite(mean))
