"""The panel launches of a teacher-forced pass (wm_set_teacher_panel) one by one, through the debug library's hooks: a panel is
C windows x w consecutive positions p0 .. p0 + w - 1, row r = c * w + s.  Every comparison is against the STEP path's own
launches, position by position, on the raw bits: a panel changes which rows share a launch, never a row's arithmetic.
Geometry: tiny.en (d 384, 6 heads, 448 positions)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 448
D, H6 = 384, 6
WIDTHS = (1, 2, 3, 5, 8)
SENT16 = np.uint32(0x7fc50000)   # WMDBG_SENTINEL_BF16 widened to f32
SENT32 = np.uint32(0x7fc0dead)   # WMDBG_SENTINEL_F32


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
    lib.wmdbg_dec_attention.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.wmdbg_dec_self_attention_panel.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    lib.wmdbg_dec_gemv_ln.argtypes = [vp, ip] + [vp] * 5 + [ip] * 7 + [vp] * 8
    lib.wmdbg_dec_qkv_panel.argtypes = [vp] * 6 + [ip] * 7 + [vp] * 3
    lib.wmdbg_dec_embed_panel.argtypes = [vp, vp, vp, ip, ip, ip, vp] + [ip] * 6 + [vp] * 4
    lib.wmdbg_align_capture_panel.argtypes = [vp, vp, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, vp]
    lib.wmdbg_align_token_prob_panel.argtypes = [vp, vp, ip, ip, ip, ip, vp, ip, ip, ip, ip, vp, ip, ip, vp]
    yield c
    c.close()


def ok(dbg, st):
    assert st == 0, dbg.lib.wm_last_error()


# ---------------------------------------------------------------- 1. self-attention
def _p0s(w):
    """panels that straddle every block boundary of the 4-stream deal (a stream's block is 128 keys, a stream's share of
    it 32): key counts p0 + s + 1 around 1, 32, 128, 256 and 441 .. 448"""
    want = {0, 31 - w // 2, 32, 127 - w // 2, 128, 255 - w // 2, 256, T - 8, T - w}
    return sorted(p for p in want if 0 <= p and p + w <= T)


@pytest.mark.parametrize("C,H", [(1, 1), (3, 1), (1, 6), (3, 6)])
def test_self_attention_panel_rows_are_the_step_kernels(dbg, C, H):
    rng = np.random.default_rng(100 * C + H)
    k = bf(rng.standard_normal((C, H, T, 64)))
    v = bf(rng.standard_normal((C, H, T, 64)) + np.linspace(-1, 1, 64))

    def step(q_rows, pos):
        kk, vv = k.copy(), v.copy()
        kk[:, :, pos + 1:] = 1e3      # what a step has not appended yet: anything
        vv[:, :, pos + 1:] = np.nan
        out = np.zeros((C, H * 64), np.float32)
        ok(dbg, dbg.lib.wmdbg_dec_attention(dbg.handle, P(q_rows), P(kk), P(vv), C, H, T, pos + 1, 0, P(out)))
        return out

    for w in WIDTHS:
        for p0 in _p0s(w):
            q = rng.standard_normal((C * w, H * 64)).astype(np.float32)
            kk, vv = k.copy(), v.copy()
            kk[:, :, p0 + w:] = 1e3   # the panel's QKV launch has appended positions p0 .. p0 + w - 1: the LATER ones of a
            vv[:, :, p0 + w:] = np.nan  # row are real values the causal mask must hide, behind them anything
            rows = ((C * w + 15) // 16) * 16 + 16
            out = np.zeros((rows, H * 64), np.float32)
            ok(dbg, dbg.lib.wmdbg_dec_self_attention_panel(dbg.handle, P(q), P(kk), P(vv), C, w, H, T, p0, rows, P(out)))
            assert np.all(bits(out[C * w:]) == SENT16), (w, p0)
            assert np.isfinite(out[:C * w]).all(), (w, p0)
            for s in range(w):
                want = step(np.ascontiguousarray(q[s::w]), p0 + s)
                assert np.array_equal(bits(out[s:C * w:w]), bits(want)), (w, p0, s)


def test_self_attention_panel_of_128_rows(dbg):
    """16 windows x 8 positions x 6 heads = 768 pairs: more workgroups than CUs"""
    C, H, w, p0 = 16, 6, 8, 200
    rng = np.random.default_rng(5)
    k = bf(rng.standard_normal((C, H, T, 64)))
    v = bf(rng.standard_normal((C, H, T, 64)))
    q = rng.standard_normal((C * w, H * 64)).astype(np.float32)
    out = np.zeros((C * w + 16, H * 64), np.float32)
    ok(dbg, dbg.lib.wmdbg_dec_self_attention_panel(dbg.handle, P(q), P(k), P(v), C, w, H, T, p0, C * w + 16, P(out)))
    assert np.all(bits(out[C * w:]) == SENT16)
    for s in (0, 3, 7):
        want = np.zeros((C, H * 64), np.float32)
        ok(dbg, dbg.lib.wmdbg_dec_attention(dbg.handle, P(np.ascontiguousarray(q[s::w])), P(k), P(v), C, H, T, p0 + s + 1, 0, P(want)))
        assert np.array_equal(bits(out[s:C * w:w]), bits(want)), s


def test_self_attention_panel_rejects_bad_geometry(dbg):
    z = np.zeros(1 << 16, np.float32)
    for C, w, p0 in ((1, 9, 0), (1, 0, 0), (17, 8, 0), (1, 8, T - 7)):
        assert dbg.lib.wmdbg_dec_self_attention_panel(dbg.handle, P(z), P(z), P(z), C, w, 1, T, p0, 144, P(z)) == 1


# ---------------------------------------------------------------- 2. QKV append
@pytest.mark.parametrize("C,w,pos", [(1, 8, 0), (3, 5, 0), (3, 2, 445), (16, 8, 440), (5, 3, 7), (2, 1, 447), (6, 3, 100)])
def test_qkv_panel_append_equals_w_step_launches(dbg, C, w, pos):
    rng = np.random.default_rng(1000 * C + 10 * w + pos)
    N, K, Bn = 3 * D, D, C * w
    x = (rng.standard_normal((Bn, K)) * 0.7 + rng.standard_normal((Bn, 1))).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    W = bf(rng.standard_normal((N, K)) * 0.05)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    q = np.zeros((Bn, D), np.float32)
    kc = np.zeros((C, H6, T, 64), np.float32)
    vc = np.zeros_like(kc)
    ok(dbg, dbg.lib.wmdbg_dec_qkv_panel(dbg.handle, P(x), P(g), P(beta), P(W), P(bias), C, w, N, K, H6, T, pos, P(q), P(kc), P(vc)))
    want_k = np.full(kc.shape, 0, np.float32).view(np.uint32)
    want_k[...] = SENT16
    want_v = want_k.copy()
    npad = (N + 15) // 16 * 16
    Wf, c1, c2 = np.zeros((npad, K), np.float32), np.zeros(npad, np.float32), np.zeros(npad, np.float32)
    for s in range(w):
        xs = np.ascontiguousarray(x[s::w])
        q1 = np.zeros((C, D), np.float32)
        k1 = np.zeros((C, H6, T, 64), np.float32)
        v1 = np.zeros_like(k1)
        mean = np.zeros(C, np.float32)
        ok(dbg, dbg.lib.wmdbg_dec_gemv_ln(dbg.handle, 0, P(xs), P(g), P(beta), P(W), P(bias), C, N, K, 1, H6, T, pos + s, P(q1), None,
                                          P(k1), P(v1), P(mean), P(Wf), P(c1), P(c2)))
        assert np.array_equal(bits(q[s::w]), bits(q1)), s
        others = np.ones(T, bool)
        others[pos + s] = False
        assert np.all(bits(k1)[:, :, others] == SENT16) and np.all(bits(v1)[:, :, others] == SENT16)
        want_k[:, :, pos + s] = bits(k1)[:, :, pos + s]
        want_v[:, :, pos + s] = bits(v1)[:, :, pos + s]
    assert not np.any(want_k[:, :, pos:pos + w] == SENT16)
    # the appended C x w rows equal the steps', every other element of the caches keeps its canary
    assert np.array_equal(bits(kc), want_k)
    assert np.array_equal(bits(vc), want_v)


# ---------------------------------------------------------------- 3. embedding
@pytest.mark.parametrize("stride,c0,C,w,pos", [(5, 1, 3, 8, 0), (17, 16, 1, 5, 443), (16, 0, 16, 8, 8), (3, 0, 3, 1, 0),
                                                (3, 2, 1, 2, 0), (20, 3, 17, 7, 1)])
def test_embed_panel_equals_the_step_paths_embeddings(dbg, stride, c0, C, w, pos):
    rng = np.random.default_rng(stride * 100 + w + pos)
    V, n_ctx = 1000, T
    emb = bf(rng.standard_normal((V, D)) * 0.1)
    pemb = (rng.standard_normal((n_ctx, D)) * 0.1 + 0.5).astype(np.float32)
    seq = rng.integers(0, V, size=(n_ctx, stride)).astype(np.int32)
    got = []
    for by_steps in (0, 1):
        x = np.zeros((C * w, D), np.float32)
        xb = np.zeros((C * w, D), np.float32)
        st = np.zeros((C * w, D // 16, 2), np.float32)
        mean = np.zeros(C * w, np.float32)
        ok(dbg, dbg.lib.wmdbg_dec_embed_panel(dbg.handle, P(emb), P(pemb), V, D, n_ctx, P(seq), stride, c0, C, w, pos, by_steps, P(x),
                                              P(xb), P(st), P(mean)))
        got.append((x, xb, st, mean))
    for a, b_, name in zip(got[0], got[1], ("x", "xb", "stats", "mean")):
        assert np.array_equal(bits(a), bits(b_)), name
    x, xb, st, mean = got[0]
    for c in range(C):     # ... and they are the rows asked for
        for s in range(w):
            want = emb[seq[pos + s, c0 + c]] + pemb[pos + s]
            assert np.array_equal(x[c * w + s], want), (c, s)
    assert np.all(st[:, 1:] == 0) and np.all(np.isfinite(st)) and np.all(np.isfinite(xb)) and np.all(np.isfinite(mean))


# ---------------------------------------------------------------- 4. query capture and token probability
@pytest.mark.parametrize("C,w,pos,Tq", [(3, 8, 8, 13), (1, 5, 0, 5), (16, 8, 0, 21), (2, 3, 10, 30), (4, 1, 2, 9)])
def test_align_capture_panel_equals_the_step_launches(dbg, C, w, pos, Tq):
    rng = np.random.default_rng(C * 100 + w + pos)
    dq = rng.standard_normal((C * w, D)).astype(np.float32)
    heads = np.array([1, 4], np.int32)
    J, slot0 = 6, 2
    caps = []
    for by_steps in (0, 1):
        cap = np.zeros((C, Tq, J, 64), np.float32)
        ok(dbg, dbg.lib.wmdbg_align_capture_panel(dbg.handle, P(dq), D, C, w, pos, P(heads), 2, slot0, Tq, J, by_steps, P(cap)))
        caps.append(cap)
    assert np.array_equal(bits(caps[0]), bits(caps[1]))
    want = np.zeros((C, Tq, J, 64), np.float32).view(np.uint32)
    want[...] = SENT32
    for c in range(C):
        for s in range(w):
            if pos + s < Tq:   # (a row at a position >= Tq is not captured)
                for j, h in enumerate(heads):
                    want[c, pos + s, slot0 + j] = bits(dq[c * w + s, h * 64:(h + 1) * 64])
    assert np.array_equal(bits(caps[0]), want)


@pytest.mark.parametrize("w,pos", [(8, 0), (5, 3), (3, 1), (1, 4), (8, 6)])
def test_align_token_prob_panel_equals_the_step_launches(dbg, w, pos):
    """chunk 0 has no text, chunk 1 a text shorter than the panel, chunk 3 one that outlasts it"""
    C, V, ldo, S, eot, n_ctx, max_text = 4, 1000, 1008, 3, 890, 32, 12
    n_text = np.array([0, 2, 7, 12], np.int32)
    rng = np.random.default_rng(10 * w + pos)
    logits = (rng.standard_normal((C * w, ldo)) * 3).astype(np.float32)
    seq = rng.integers(0, eot, size=(n_ctx, C)).astype(np.int32)
    probs = []
    for by_steps in (0, 1):
        prob = np.zeros((C, max_text), np.float32)
        ok(dbg, dbg.lib.wmdbg_align_token_prob_panel(dbg.handle, P(logits), C, w, V, ldo, P(seq), n_ctx, pos, S, eot, P(n_text), max_text,
                                                     by_steps, P(prob)))
        probs.append(prob)
    assert np.array_equal(bits(probs[0]), bits(probs[1]))
    written = bits(probs[0]) != SENT32
    for c in range(C):
        for i in range(max_text):
            p = S + i
            mine = i < n_text[c] and pos <= p < pos + w
            assert written[c, i] == mine, (c, i)
            if mine:
                row = logits[c * w + p - pos, :eot].astype(np.float64)
                want = np.exp(row[seq[p + 1, c]] - row.max()) / np.exp(row - row.max()).sum()
                assert abs(probs[0][c, i] - want) <= 1e-5 * want + 1e-12
    assert not written[0].any() and written[1].sum() == len([i for i in range(2) if pos <= S + i < pos + w])
