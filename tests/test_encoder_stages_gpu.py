"""The product's own encoder-side launches on a loaded model, stage by stage and element by element: the stem (mel re-layout,
conv1, conv2 as wm_model_encode_win launches them, on the conv weights as wm_set_tensor packed them), one layer's LayerNorm +
QKV launch (pre-scaled queries, keys, V^T in the attention kernel's column order), the rest of the layer (attention, out-
projection, LayerNorm, fc1 + GELU, fc2), ln_post and the cross-K/V scatter, through wmdbg_encode_stem / wmdbg_encode_layer_qkv /
wmdbg_encode_layer_tail / wmdbg_encode_post / wmdbg_cross_kv.  B = 3: the chunk boundaries at rows 1500 and 3000 (3000 and 6000
for conv1) are no multiple of 64, 128 or 256.  Every stage is measured on the DEVICE's own input to it.  References and bounds:
tests/enc_gemm_ref.py (float64; delta = 2 K u S), tests/enc_attn_ref.py, tests/layernorm_ref.py.
Whole-model rel-L2 (test_model_gpu.py) does not see one misplaced frame per chunk; these do."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_attn_ref as E   # noqa: E402
import enc_gemm_ref as R   # noqa: E402
import layernorm_ref as L   # noqa: E402

pytestmark = pytest.mark.gpu

W = importlib.import_module("openai_whisper_coreml_amd.weights")
TINY = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=2,
            n_vocab=1024, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=2)
TILES = ((64, 0), (128, 1), (128, 2), (256, 0))
B, S, T = 3, 1500, 3000
_WORST = {}


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def nontrivial_ln(sd, seed=0):
    """Synthetic weights have LN gamma = 1, beta = 0; perturb so that the LN parameters are exercised (as test_model_gpu.py)."""
    rng = np.random.default_rng(seed)
    for k in sd:
        if "ln" in k and k.endswith("weight"):
            sd[k] = (1 + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
        if "ln" in k and k.endswith("bias"):
            sd[k] = (0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    return sd


class Model:
    def __init__(self, pkg, n_mels):
        self.dims = dict(TINY, n_mels=n_mels)
        self.sd = nontrivial_ln(W.synthetic_state_dict(self.dims, seed=11, matrix_gain=4.0))
        self.ctx = c = pkg.binding.Context(self.dims, debug=True)
        c.load_state_dict(self.sd)
        c.finalize()
        vp, ip = ctypes.c_void_p, ctypes.c_int
        c.lib.wmdbg_encode_stem.argtypes = [vp, vp, vp, ip, vp, vp, vp]
        c.lib.wmdbg_encode_layer_qkv.argtypes = [vp, ip, vp, ip, vp, vp, vp]
        c.lib.wmdbg_encode_layer_tail.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, vp]
        c.lib.wmdbg_encode_post.argtypes = [vp, vp, ip, vp, vp]
        c.lib.wmdbg_cross_kv.argtypes = [vp, vp, ip, vp]
        c.lib.wmdbg_set_gemm_tile.argtypes = [ctypes.c_int]
        c.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
        c.lib.wm_last_error.restype = ctypes.c_char_p
        self.C, self.d, self.H = n_mels, 128, 2
        rng = np.random.default_rng(n_mels)
        self.mel = (rng.standard_normal((B, n_mels, T)) + np.linspace(-1, 1, n_mels)[None, :, None]).astype(np.float32)
        self.x = (rng.standard_normal((B * S, self.d)) * 3 + 1.5).astype(np.float32)
        self.xa = (rng.standard_normal((B, S, self.d)) + np.linspace(-0.5, 0.5, self.d)).astype(np.float32)

    def tile(self, tile, pipe):
        assert self.ctx.lib.wmdbg_set_gemm_tile(tile) == 0
        assert self.ctx.lib.wmdbg_set_tuning(b"gemm128_pipe", pipe) == 0

    def reset(self):
        self.ctx.lib.wmdbg_set_gemm_tile(0)
        self.ctx.lib.wmdbg_set_tuning(b"reset", 0)

    def stem(self, mel, wins=None, n=None):
        n = len(mel) if n is None else n
        mel_t = np.zeros((n, T + 2, self.C), np.float32)
        h1p = np.zeros((n, T + 1, self.d), np.float32)
        x = np.zeros((n, S, self.d), np.float32)
        st = self.ctx.lib.wmdbg_encode_stem(self.ctx.handle, P(np.ascontiguousarray(mel, np.float32)), P(wins), n, P(mel_t), P(h1p), P(x))
        assert st == 0, self.ctx.lib.wm_last_error()
        return mel_t, h1p, x

    def layer_qkv(self, layer, x):
        n = len(x) // S
        xn = np.zeros((n * S, self.d), np.float32)
        qk = np.zeros((n * S, 2 * self.d), np.float32)
        vt = np.zeros((n, self.H, 64, 1536), np.float32)
        st = self.ctx.lib.wmdbg_encode_layer_qkv(self.ctx.handle, layer, P(np.ascontiguousarray(x, np.float32)), n, P(xn), P(qk), P(vt))
        assert st == 0, self.ctx.lib.wm_last_error()
        return xn, qk, vt

    def layer_tail(self, layer, x):
        """-> att, x_mid, xn2, hid, x_out; NaN where the hook wrote nothing"""
        n = len(x) // S
        outs = [np.full((n * S, w), np.nan, np.float32) for w in (self.d, self.d, self.d, 4 * self.d, self.d)]
        st = self.ctx.lib.wmdbg_encode_layer_tail(self.ctx.handle, layer, P(np.ascontiguousarray(x, np.float32)), n, *[P(o) for o in outs])
        assert st == 0, self.ctx.lib.wm_last_error()
        return outs

    def post(self, x):
        n = len(x) // S
        xn, xa = (np.full((n * S, self.d), np.nan, np.float32) for _ in range(2))
        st = self.ctx.lib.wmdbg_encode_post(self.ctx.handle, P(np.ascontiguousarray(x, np.float32)), n, P(xn), P(xa))
        assert st == 0, self.ctx.lib.wm_last_error()
        return xn, xa

    def cross_kv(self, xa):
        n = len(xa)
        out = np.zeros((self.dims["n_text_layer"], 2, n, self.H, S, 64), np.float32)
        st = self.ctx.lib.wmdbg_cross_kv(self.ctx.handle, P(np.ascontiguousarray(xa, np.float32)), n, P(out))
        assert st == 0, self.ctx.lib.wm_last_error()
        return out


@pytest.fixture(scope="module", params=[80, 128], ids=["mels80", "mels128"])
def model(pkg, request):
    m = Model(pkg, request.param)
    yield m
    m.reset()
    m.ctx.close()
    for k in sorted(_WORST):          # (shown with -s) largest |got - ref| / bound per stage output
        print("error / bound, n_mels %d, %-6s %.4f" % (request.param, k, _WORST[k]))
    _WORST.clear()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within(name, got, ref, bnd):
    ratio = np.abs(got.astype(np.float64) - ref) / bnd
    assert np.isfinite(ratio).all(), name + ": an element is not finite (never written?)"
    worst = float(ratio.max())
    print("%s: error / bound = %.4f" % (name, worst))
    _WORST[name] = max(_WORST.get(name, 0.0), worst)
    assert worst <= 1.0, (name, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


def check_stem(m, mel, mel_t, h1p, x, tag):
    sd = m.sd
    want_t = R.time_major(R.bf16(mel))
    assert np.array_equal(bits(mel_t), bits(want_t)), tag            # the re-layout is exact; guard rows 0 and 3001 are zero
    assert not bits(mel_t[:, 0]).any() and not bits(mel_t[:, T + 1]).any()
    assert not bits(h1p[:, 0]).any(), tag                              # conv2's zero pad row in front of every chunk
    k1pad = (3 * m.C + 63) // 64 * 64
    ref1, S1 = R.conv1_ref(R.bf16(mel), R.bf16(sd["encoder.conv1.weight"]), sd["encoder.conv1.bias"])
    g1 = R.Geom(K=k1pad, epi=R.EPI_GELU_BF16)
    within("h1p", h1p[:, 1:], ref1, R.bound(g1, ref1, S1))
    # conv2 on the DEVICE's own h1p: only conv2 is measured
    ref2, S2 = R.conv2_ref(h1p[:, 1:], R.bf16(sd["encoder.conv2.weight"]), sd["encoder.conv2.bias"],
                           sd["encoder.positional_embedding"])
    g2 = R.Geom(K=3 * m.d, epi=R.EPI_CONV2_F32)
    within("x", x, ref2, R.bound(g2, ref2, S2))


def test_stem_every_element_through_every_tile(model):
    m = model
    try:
        outs = []
        for tile, pipe in TILES:
            m.tile(tile, pipe)
            mel_t, h1p, x = m.stem(m.mel)
            check_stem(m, m.mel, mel_t, h1p, x, (tile, pipe))
            outs.append((h1p, x))
        for o in outs[1:]:                                             # same accumulation order in every tile
            assert np.array_equal(bits(o[0]), bits(outs[0][0])) and np.array_equal(bits(o[1]), bits(outs[0][1]))
    finally:
        m.reset()


def test_stem_mel_windows(model):
    """wm_transcribe_mel's window form: frames seek .. seek + n - 1 of a [C][T] block, zeros from n to 3000; five windows of two
    blocks in one call.  The re-layout is exact, and conv1 / conv2 behind it give the bits of the materialised windows."""
    m = model
    rng = np.random.default_rng(7)
    T1, T2 = 7000, 3100
    blk1 = (rng.standard_normal((m.C, T1)) + np.linspace(-1, 1, m.C)[:, None]).astype(np.float32)
    blk2 = (rng.standard_normal((m.C, T2)) - 0.5).astype(np.float32)
    base2 = m.C * T1 + 5
    buf = np.concatenate([blk1.ravel(), np.full(5, 1e30, np.float32), blk2.ravel()])
    rows = [(blk1, 0, T1, 0, 3000), (blk1, 0, T1, 4000, 3000), (blk1, 0, T1, 6990, 10), (blk1, 0, T1, 123, 2999),
            (blk2, base2, T2, 64, 64)]
    wins = np.array([r[1:] for r in rows], np.int64)
    mat = np.stack([R.mel_window(r[0], r[3], r[4]) for r in rows])
    mel_t, h1p, x = m.stem(buf, wins, n=len(rows))
    assert np.array_equal(bits(mel_t), bits(R.time_major(R.bf16(mat))))
    mel_t2, h1p2, x2 = m.stem(mat)
    assert np.array_equal(bits(mel_t), bits(mel_t2)) and np.array_equal(bits(h1p), bits(h1p2)) and np.array_equal(bits(x), bits(x2))
    check_stem(m, mat, mel_t, h1p, x, "windows")


def test_stem_rejects_a_window_that_leaves_its_block(model):
    m = model
    buf = np.zeros(m.C * 3000, np.float32)
    for bad in ([0, 3000, 1, 3000], [0, 3000, 0, 3001], [-1, 3000, 0, 10], [0, 0, 0, 0]):
        out = [np.zeros(1, np.float32)] * 3
        st = m.ctx.lib.wmdbg_encode_stem(m.ctx.handle, P(buf), P(np.array([bad], np.int64)), 1, P(out[0]), P(out[1]), P(out[2]))
        assert st == 1 and b"window" in m.ctx.lib.wm_last_error()


def qkv_weights(sd, prefix, d):
    w = np.concatenate([sd[prefix + ".query.weight"], sd[prefix + ".key.weight"], sd[prefix + ".value.weight"]])
    b = np.concatenate([sd[prefix + ".query.bias"], np.zeros(d, np.float32), sd[prefix + ".value.bias"]])
    return R.bf16(w), b


@pytest.mark.parametrize("layer", [0, 1])
def test_layer_qkv_every_element_through_every_tile(model, layer):
    m = model
    sd = m.sd
    pre = "encoder.blocks.%d" % layer
    ln = torch.nn.functional.layer_norm(torch.from_numpy(m.x).double(), (m.d,), torch.from_numpy(sd[pre + ".attn_ln.weight"]).double(),
                                        torch.from_numpy(sd[pre + ".attn_ln.bias"]).double(), 1e-5).numpy()
    Wq, bq = qkv_weights(sd, pre + ".attn", m.d)
    g = R.qkv_geom(m.d, m.H, S, B, K=m.d)
    assert g.seq_pad == 1536
    try:
        outs = []
        for tile, pipe in TILES:
            m.tile(tile, pipe)
            xn, qk, vt = m.layer_qkv(layer, m.x)
            assert np.abs(xn - ln).max() <= 2 ** -8 * np.abs(ln).max() + 1e-6          # test_layernorm's bf16 tolerance
            # the product of the DEVICE's xn: only the QKV launch is measured; exact layout, sentinels in the pad columns
            ref, Sb = R.values(g, xn, Wq, bq)
            worst = R.scatter_check(g, qk, vt, ref, Sb)
            print("qkv layer %d tile %s: error / bound = %.4f" % (layer, (tile, pipe), worst))
            _WORST["qk_vt"] = max(_WORST.get("qk_vt", 0.0), worst)
            assert worst <= 1.0
            assert (bits(vt)[..., S:] == R.SENT_BF16).all()
            outs.append((xn, qk, vt))
        for o in outs[1:]:
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(o, outs[0]))
        # the hook leaves the pad columns zero again: a following encode still works and is finite
        assert np.isfinite(m.ctx.encode_mel(m.mel[:1])).all()
    finally:
        m.reset()


def attention_operands(m, qk, vt):
    """(pre-scaled queries, keys, values) [n][S][d] of the returned qk / vt: wm_att_vt_pos undone by enc_gemm_ref's restatement"""
    n = len(qk) // S
    qs, k = qk[:, :m.d].reshape(n, S, m.d), qk[:, m.d:].reshape(n, S, m.d)
    v = vt[:, :, :, R.vt_pos(np.arange(S))].transpose(0, 3, 1, 2).reshape(n, S, m.d)
    return qs, k, v


@pytest.mark.parametrize("layer", [0, 1])
def test_layer_tail_every_element_through_every_tile(model, layer):
    """attention, out-projection + residual, LayerNorm, fc1 + GELU, fc2 + residual as wm_model_encode_layer_tail launches them"""
    m = model
    sd = m.sd
    pre = "encoder.blocks.%d" % layer
    M = B * S
    Wo, W1, W2 = (R.bf16(sd[pre + k]) for k in (".attn.out.weight", ".mlp.0.weight", ".mlp.2.weight"))
    g_o, g_1, g_2 = R.plain(M, m.d, m.d, R.EPI_RESID_F32), R.plain(M, 4 * m.d, m.d, R.EPI_GELU_BF16), R.plain(M, m.d, 4 * m.d, R.EPI_RESID_F32)
    try:
        outs, att_ref, first_qk = [], None, None
        for tile, pipe in TILES:
            m.tile(tile, pipe)
            _, qk, vt = m.layer_qkv(layer, m.x)
            att, x_mid, xn2, hid, x_out = m.layer_tail(layer, m.x)
            if att_ref is None or not (np.array_equal(bits(qk), bits(first_qk[0])) and np.array_equal(bits(vt), bits(first_qk[1]))):
                first_qk = (qk, vt)
                qs, k, v = attention_operands(m, qk, vt)      # (no pad column among the 1500 live ones: all finite)
                assert np.isfinite(v).all()
                att_ref = E.restate(None, k, v, m.H, qs=qs)
            within("att", att, att_ref.ref.reshape(M, m.d), att_ref.bound[0].reshape(M, m.d))
            ref, Sb = R.values(g_o, att, Wo, sd[pre + ".attn.out.bias"], C0=m.x)
            within("x_mid", x_mid, ref, R.bound(g_o, ref, Sb))
            y, bnd = L.restate(x_mid, sd[pre + ".mlp_ln.weight"], sd[pre + ".mlp_ln.bias"])
            lo, hi = L.bf16_bracket(y, bnd)
            assert ((lo <= xn2) & (xn2 <= hi)).all(), ("xn2", np.argwhere(~((lo <= xn2) & (xn2 <= hi)))[:5])
            ref, Sb = R.values(g_1, xn2, W1, sd[pre + ".mlp.0.bias"])
            within("hid", hid, ref, R.bound(g_1, ref, Sb))
            ref, Sb = R.values(g_2, hid, W2, sd[pre + ".mlp.2.bias"], C0=x_mid)
            within("x_out", x_out, ref, R.bound(g_2, ref, Sb))
            outs.append((att, x_mid, xn2, hid, x_out))
        for o in outs[1:]:                                             # same accumulation order in every tile
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(o, outs[0]))
        # the hook leaves the buffers as a later encode expects them
        assert np.isfinite(m.ctx.encode_mel(m.mel[:1])).all()
    finally:
        m.reset()


def test_post_every_element(model):
    """ln_post as wm_model_encode_post launches it (both outputs), on the residual stream and on one with an outlier column"""
    m = model
    g, b = m.sd["encoder.ln_post.weight"], m.sd["encoder.ln_post.bias"]
    spike = m.x.copy()
    spike[:, 5] *= 1e3
    for name, x in (("xa", m.x), ("xa_spike", spike)):
        xn, xa = m.post(x)
        y, bnd = L.restate(x, g, b)
        within(name, xa, y, bnd)
        assert np.array_equal(bits(xn), bits(L.bf16(xa))), "ln_post: the bf16 output is not RNE of the f32 output"


def test_cross_kv_every_element_through_every_tile(model):
    m = model
    sd = m.sd
    g = R.xkv_geom(m.d, m.H, S, B, K=m.d)
    xa16 = R.bf16(m.xa).reshape(B * S, m.d)
    refs = []
    for l in range(m.dims["n_text_layer"]):
        pre = "decoder.blocks.%d.cross_attn" % l
        w = R.bf16(np.concatenate([sd[pre + ".key.weight"], sd[pre + ".value.weight"]]))
        b = np.concatenate([np.zeros(m.d, np.float32), sd[pre + ".value.bias"]])       # the key half has no bias
        refs.append(R.values(g, xa16, w, b))
    try:
        outs = []
        for tile, pipe in TILES:
            m.tile(tile, pipe)
            xkv = m.cross_kv(m.xa)
            for l, (ref, Sb) in enumerate(refs):
                worst = R.scatter_check(g, xkv[l].ravel(), None, ref, Sb)
                print("xkv layer %d tile %s: error / bound = %.4f" % (l, (tile, pipe), worst))
                _WORST["xkv"] = max(_WORST.get("xkv", 0.0), worst)
                assert worst <= 1.0
            outs.append(xkv)
        for o in outs[1:]:
            assert np.array_equal(bits(o), bits(outs[0]))
    finally:
        m.reset()


def test_chunk_one_of_three_is_bit_identical_to_the_chunk_alone(model):
    """Chunks are independent units: the stage outputs of chunk 1 of 3 carry the bits of the same chunk encoded alone."""
    m = model
    _, h1p3, x3 = m.stem(m.mel)
    _, h1p1, x1 = m.stem(m.mel[1:2])
    assert np.array_equal(bits(h1p3[1]), bits(h1p1[0])) and np.array_equal(bits(x3[1]), bits(x1[0]))
    xn3, qk3, vt3 = m.layer_qkv(1, m.x)
    xn1, qk1, vt1 = m.layer_qkv(1, m.x[S:2 * S])
    assert np.array_equal(bits(xn3[S:2 * S]), bits(xn1))
    assert np.array_equal(bits(qk3[S:2 * S]), bits(qk1)) and np.array_equal(bits(vt3[1]), bits(vt1[0]))
    for a3, a1 in zip(m.layer_tail(1, m.x) + list(m.post(m.x)), m.layer_tail(1, m.x[S:2 * S]) + list(m.post(m.x[S:2 * S]))):
        assert np.array_equal(bits(a3[S:2 * S]), bits(a1))
    xkv3 = m.cross_kv(m.xa)
    xkv1 = m.cross_kv(m.xa[1:2])          # (the model's cache is still sized for 3 chunks: the hook checks that rows 1, 2 stay untouched)
    assert np.array_equal(bits(xkv3[:, :, 1]), bits(xkv1[:, :, 0]))
