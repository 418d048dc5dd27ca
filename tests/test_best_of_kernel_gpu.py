"""GPU test of the candidate-group cross-attention (dec_xcand_attn_kernel through wmdbg_dec_attention_cand, the launch
wm_model_decode_step makes for a wm_transcribe_mel_best_of group): C windows x N candidates read each window's K/V once.
Contract: row c * N + s gets, BIT FOR BIT, what the single-query cross-attention launch (wmdbg_dec_attention, nsplit -1)
gives that query over a copy of window c's K/V -- for every N, with all rows live and with a live list that has lost single
candidates and whole windows."""
import ctypes
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = importlib.import_module("openai_whisper_coreml_amd.weights")


def bf(x):
    return W.bf16_round_f32(np.ascontiguousarray(x, dtype=np.float32))


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.binding.Context(debug=True)
    vp, ip = ctypes.c_void_p, ctypes.c_int
    c.lib.wmdbg_dec_attention.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    c.lib.wmdbg_dec_attention_cand.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    c.lib.wmdbg_dec_attention_cand_shared.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    yield c
    c.close()


def _live_list(C, N, rng):
    """every window keeps a random subset of its candidates; some windows lose all of them, some keep all"""
    live = []
    for c in range(C):
        mode = c % 4
        if mode == 1 and C > 1:
            continue                       # a whole window has finished
        keep = np.ones(N, bool) if mode == 3 else rng.random(N) < 0.6
        if not keep.any():
            keep[rng.integers(N)] = True
        live += [c * N + s for s in range(N) if keep[s]]
    return np.array(live, dtype=np.int32)


# Launch shapes: below 256 (window, head) pairs the flat deal + combine launch -- (1, 1, 6), (1, 5, 6), (8, 5, 20), (25, 5, 8);
# from 256 pairs the persistent 8-wave workgroups with the merge in LDS, candidates in ONE pass (24, 5, 20: the shape of a
# 24-window best_of 5 group at 20 heads; 13, 3, 20) and in TWO passes (16, 8, 20; 21, 6, 13).  Every shape is also run as the
# decode step launches it when the chip is shared (short-lived workgroups, LDS merge whatever the pair count).
@pytest.mark.parametrize("C,N,H", [(1, 1, 6), (1, 5, 6), (8, 5, 20), (25, 5, 8), (16, 8, 20), (24, 5, 20), (13, 3, 20), (21, 6, 13)])
@pytest.mark.parametrize("n_keys", [1500, 437])
def test_candidates_get_the_single_query_bits(ctx, C, N, H, n_keys):
    T = 1500
    rng = np.random.default_rng(1000 * C + 10 * N + H + n_keys)
    B = C * N
    q = rng.standard_normal((B, H * 64)).astype(np.float32)
    k = bf(rng.standard_normal((C, H, T, 64)))
    v = bf(rng.standard_normal((C, H, T, 64)) + np.linspace(-1, 1, 64))
    k[:, :, n_keys:] = np.nan    # what the product leaves there is uninitialised: NaN in K and in V must be harmless
    v[:, :, n_keys:] = np.nan
    want = np.zeros((B, H * 64), np.float32)
    kr, vr = np.repeat(k, N, axis=0), np.repeat(v, N, axis=0)   # every window's K/V once per candidate
    assert ctx.lib.wmdbg_dec_attention(ctx.handle, P(q), P(kr), P(vr), B, H, T, n_keys, -1, P(want)) == 0, ctx.lib.wm_last_error()
    del kr, vr
    assert np.isfinite(want).all() and np.abs(want).max() > 0.1
    # every row live (no live list, and the full list)
    full = np.arange(B, dtype=np.int32)
    for lr in (None, full):
        got = np.full((B, H * 64), -7.0, np.float32)
        st = ctx.lib.wmdbg_dec_attention_cand(ctx.handle, P(q), P(k), P(v), C, N, H, T, n_keys, P(lr) if lr is not None else None,
                                              B, P(got))
        assert st == 0, ctx.lib.wm_last_error()
        assert np.array_equal(got, want), (C, N, H, n_keys, lr is None)
    # single candidates and whole windows gone
    live = _live_list(C, N, rng)
    got = np.zeros((B, H * 64), np.float32)
    st = ctx.lib.wmdbg_dec_attention_cand(ctx.handle, P(q), P(k), P(v), C, N, H, T, n_keys, P(live), live.size, P(got))
    assert st == 0, ctx.lib.wm_last_error()
    assert np.array_equal(got[live], want[live]), (C, N, H, n_keys, live.tolist())
    # the shape of a burst that shares the chip: all rows, then the thinned list
    for lr in (None, live):
        got = np.zeros((B, H * 64), np.float32)
        st = ctx.lib.wmdbg_dec_attention_cand_shared(ctx.handle, P(q), P(k), P(v), C, N, H, T, n_keys,
                                                     P(lr) if lr is not None else None, B if lr is None else lr.size, P(got))
        assert st == 0, ctx.lib.wm_last_error()
        rows = full if lr is None else lr
        assert np.array_equal(got[rows], want[rows]), (C, N, H, n_keys, "shared", lr is None)


def test_bad_arguments_are_rejected(ctx):
    q = np.zeros((8, 64), np.float32)
    k = np.zeros((1, 1, 64, 64), np.float32)
    out = np.zeros((8, 64), np.float32)
    lib = ctx.lib
    assert lib.wmdbg_dec_attention_cand(ctx.handle, P(q), P(k), P(k), 1, 9, 1, 64, 64, None, 0, P(out)) == 1    # N > 8
    assert lib.wmdbg_dec_attention_cand(ctx.handle, P(q), P(k), P(k), 17, 8, 1, 64, 64, None, 0, P(out)) == 1   # > 128 rows
    bad = np.array([3, 2], dtype=np.int32)                                                                      # not ascending
    assert lib.wmdbg_dec_attention_cand(ctx.handle, P(q), P(k), P(k), 1, 8, 1, 64, 64, P(bad), 2, P(out)) == 1
    assert b"ascending" in lib.wm_last_error()
