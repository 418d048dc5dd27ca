"""The float64 restatements of tests/enc_gemm_ref.py, checked on the CPU: the implicit-GEMM formulation of both convolutions
against torch's conv1d, the destination layouts against triple loops, vt_pos as an involution of every aligned 16-key group,
the mel window rule, and -- for the operands the exact GPU tests use -- that every value is an integer of magnitude <= 256 and
therefore exact in bf16 and in any summation order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_gemm_ref as R   # noqa: E402


def test_vt_pos_swaps_the_two_middle_groups_of_every_sixteen():
    s = np.arange(1536)
    p = R.vt_pos(s)
    assert np.array_equal(R.vt_pos(p), s)                                  # an involution
    assert np.array_equal(p // 16, s // 16)                                # inside the aligned 16-key group
    assert np.array_equal(np.sort(p.reshape(-1, 16), axis=1), s.reshape(-1, 16))   # a permutation of each group
    assert list(p[:16]) == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert np.array_equal(p % 4, s % 4)                                    # whole 4-key groups move


def test_row_map_against_a_loop():
    for (M, off, rpb, bs, rs) in [(37, 0, 38, 0, 5), (150, 64, 50, 51 * 64, 64), (21, 8, 5, 100, 16)]:
        want = [off + (m // rpb) * bs + (m % rpb) * rs for m in range(M)]
        assert list(R.row_offsets(M, off, rpb, bs, rs)) == want


def _loop_dest(g):
    ci = np.full((g.M, g.N), -1, np.int64)
    vi = np.full((g.M, g.N), -1, np.int64)
    for m in range(g.M):
        for n in range(g.N):
            if g.epi == R.EPI_XKV:
                kv, hn = divmod(n, g.d_model)
                h, e = divmod(hn, 64)
                b, s = divmod(m, g.seq)
                out = np.zeros((2, g.batch, g.n_head, g.seq, 64), np.int8)
                ci[m, n] = np.ravel_multi_index((kv, b, h, s, e), out.shape)
            elif g.epi == R.EPI_QKV_ENC and n >= 2 * g.d_model:
                h, e = divmod(n - 2 * g.d_model, 64)
                b, s = divmod(m, g.seq)
                grp, r = divmod(s, 16)
                col = grp * 16 + [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15][r]
                vi[m, n] = np.ravel_multi_index((b, h, e, col), (g.batch, g.n_head, 64, g.seq_pad))
            else:
                ci[m, n] = g.c_off + (m // g.c_rpb) * g.c_bstride + (m % g.c_rpb) * g.c_rstride + n
    return ci, vi


@pytest.mark.parametrize("g", [R.xkv_geom(128, 2, 9, 3), R.xkv_geom(64, 1, 5, 1), R.qkv_geom(128, 2, 37, 3),
                               R.qkv_geom(64, 1, 20, 1), R.batched_c(R.plain(27, 80, 64, R.EPI_F32), 5),
                               R.batched_c(R.plain(100, 64, 64, R.EPI_BIAS_BF16), 9)], ids=repr)
def test_destination_layouts_against_triple_loops(g):
    ci, vi = R.dest_index(g)
    lc, lv = _loop_dest(g)
    assert np.array_equal(ci, lc) and np.array_equal(vi, lv)
    for idx, size in ((ci, g.c_elems), (vi, g.vt_elems)):      # inside the buffer, no two outputs in one place
        w = idx[idx >= 0]
        assert w.size == 0 or (w.max() < size and np.unique(w).size == w.size)


@pytest.mark.parametrize("C,T,B", [(80, 100, 3), (128, 100, 1), (80, 37, 2)])
def test_conv1_as_an_implicit_gemm_is_conv1d(C, T, B):
    rng = np.random.default_rng(C + T)
    O = 24
    mel = rng.standard_normal((B, C, T))
    w1 = rng.standard_normal((O, C, 3)) * 0.1
    b1 = rng.standard_normal(O)
    K = (3 * C + 63) // 64 * 64
    g = R.conv1_a(R.batched_c(R.plain(B * T, O, K, R.EPI_GELU_BF16), T), C, T, B)
    vals, S = R.values(g, R.time_major(mel), R.pack_conv_weight(w1, K), b1)
    want, want_S = R.conv1_ref(mel, w1, b1)
    assert np.abs(vals - want.reshape(B * T, O)).max() <= 1e-12
    assert np.abs(S - want_S.reshape(B * T, O)).max() <= 1e-12
    # ... and its C map is the time-major buffer conv2 reads, one guard row in front of each batch
    ci, _ = R.dest_index(g)
    buf = np.zeros(g.c_elems)
    buf[ci.ravel()] = vals.ravel()
    assert np.array_equal(buf.reshape(B, T + 1, O)[:, 1:], vals.reshape(B, T, O)) and not buf.reshape(B, T + 1, O)[:, 0].any()


@pytest.mark.parametrize("d,S,B", [(64, 50, 3), (64, 50, 1), (32, 7, 2)])
def test_conv2_as_an_implicit_gemm_is_conv1d(d, S, B):
    rng = np.random.default_rng(d + S)
    O = 40
    h1 = rng.standard_normal((B, 2 * S, d))
    w2 = rng.standard_normal((O, d, 3)) * 0.1
    b2 = rng.standard_normal(O)
    pos = 1000.0 * np.arange(S)[:, None] + np.arange(O)[None, :]
    g = R.conv2_a(R.plain(B * S, O, 3 * d, R.EPI_CONV2_F32).copy(c_rpb=S, c_bstride=S * O), d, S, B)
    a_buf = R.time_major(h1.transpose(0, 2, 1), back_pad=False)
    vals, Sb = R.values(g, a_buf, R.pack_conv_weight(w2), b2, pos=pos)
    want, want_S = R.conv2_ref(h1, w2, b2, pos)
    assert np.abs(vals - want.reshape(B * S, O)).max() <= 1e-9
    assert np.abs(Sb - want_S.reshape(B * S, O)).max() <= 1e-12


def test_gelu_is_the_erf_form():
    x = np.linspace(-6, 6, 241)
    want = torch.nn.functional.gelu(torch.from_numpy(x)).numpy()
    assert np.abs(R.gelu(x) - want).max() <= 1e-15
    import math
    assert abs(R.gelu(np.array([0.7]))[0] - 0.35 * (1 + math.erf(0.7 / math.sqrt(2)))) <= 1e-16
    g = np.abs(np.diff(R.gelu(np.linspace(-8, 8, 160001)))) / 1e-4
    assert g.max() <= 1.13                                                  # the Lipschitz constant of the error bound


def test_mel_window_rule():
    blk = np.arange(3 * 7000, dtype=np.float32).reshape(3, 7000)
    for seek, n in [(0, 3000), (4000, 3000), (6990, 10), (123, 2999), (64, 64)]:
        w = R.mel_window(blk, seek, n)
        assert w.shape == (3, 3000) and not w[:, n:].any()
        for c in range(3):
            for t in (0, n // 2, n - 1):
                assert w[c, t] == blk[c, seek + t]


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 256.0, 257.0, -0.1, 3.0e38], np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.bf16(x), want)


@pytest.mark.parametrize("case", R.exact_cases(), ids=lambda c: c[0])
def test_exact_operands_give_bf16_exact_integers(case):
    """The exact GPU tests compare with array_equal: that is only a statement about placement if the arithmetic has no
    rounding at all -- every product 0 or a weight, every sum an integer of magnitude <= 256 (bf16 holds those exactly)."""
    _, g = case
    A, W, bias, C0 = R.exact_operands(g)
    assert np.array_equal(A, R.bf16(A)) and np.array_equal(W, R.bf16(W))
    vals, S = R.values(g, A, W, bias, C0=C0)
    assert np.array_equal(vals, np.round(vals)) and np.abs(vals).max() <= 256 and S.max() <= 256
    assert np.array_equal(R.bf16(vals.astype(np.float32)), vals.astype(np.float32))
    assert np.abs(vals).max() >= 64 and np.unique(vals).size > 50          # not a degenerate pattern
    rows = R.gather_rows(A, g.M, g.K, g.a_off, g.a_rpb, g.a_bstride, g.a_rstride)
    assert (np.abs(rows).sum(axis=1) > 0).mean() > 0.9                      # almost every output row sees a 1
    # neighbouring rows and columns differ, so a frame or column put one place off is seen
    assert (vals[1:] != vals[:-1]).mean() > 0.9 and (vals[:, 1:] != vals[:, :-1]).mean() > 0.9
