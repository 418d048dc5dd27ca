"""numpy / torch float64 restatement of what the encoder-side GEMM launches compute and WHERE they put it (csrc/gemm.hip,
the stem of csrc/model.cpp, mel_time_major_kernel of csrc/enc_kernels.hip), shared by test_enc_gemm_ref_cpu.py (which checks
these restatements against triple loops and torch's conv1d) and the GPU tests test_enc_gemm_kernels_gpu.py /
test_encoder_stages_gpu.py.  Nothing here is imported from the package: it is the second statement of each contract.

Row map          row m of a buffer starts at off + (m // rpb) * bstride + (m % rpb) * rstride (elements).
Epilogues        0 bias -> bf16, 1 gelu -> bf16, 2 C += (f32), 3 gelu + pos[m % c_rpb][n] (f32), 4 encoder QKV, 5 cross-K/V
                 scatter, 6 f32.  4: columns n < 2 d go to the C row (queries n < d multiplied by QSCALE in f32 before the one
                 bf16 rounding), columns n >= 2 d to vt[b][h][e][vt_pos(s)], m = b * seq + s, n - 2 d = h * 64 + e.
                 5: out[kv][b][h][s][e], n = kv * d + h * 64 + e.
vt_pos           model.h: "the two middle 4-key groups of every 16 keys are swapped": keys 4..7 <-> 8..11 of each aligned 16.
Conv stem        conv1 (k 3, pad 1) + GELU, conv2 (k 3, stride 2, pad 1) + GELU + positional embedding; as implicit GEMMs over a
                 time-major buffer with one zero row in front (and, for the mel, behind), weights packed [O][tap * C + c].
Mel window       frames seek .. seek + n - 1 of a [C][T] block, zeros from n to 3000.
Error bound      u = 2^-24, S = |A| |W|^T + |bias| in float64, delta = 2 K u S: twice the worst case of any summation order
                 (the matrix pipe's internal rounding is not documented as round-to-nearest per step)."""
import numpy as np
import torch

EPI_BIAS_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_CONV2_F32, EPI_QKV_ENC, EPI_XKV, EPI_F32 = range(7)
BF16_OUT = (EPI_BIAS_BF16, EPI_GELU_BF16, EPI_QKV_ENC, EPI_XKV)
GELU_EPI = (EPI_GELU_BF16, EPI_CONV2_F32)
QSCALE = np.float32(0.125) * np.float32(1.44269504088896340736)   # 64^-1/2 * log2(e), the f32 product model.h writes
SENT_BF16 = np.uint32(0x7fc5 << 16)    # the bf16 sentinel widened to f32 bits
SENT_F32 = np.uint32(0x7fc0dead)
U = 2.0 ** -24
N_FRAMES = 3000


def bf16(x):
    """float -> nearest-even bf16, returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def vt_pos(s):
    s = np.asarray(s, dtype=np.int64)
    g = (s >> 2) & 3                       # which 4-key group of the 16
    g2 = np.where(g == 1, 2, np.where(g == 2, 1, g))
    return (s & ~np.int64(12)) | (g2 << 2)


def row_offsets(M, off, rpb, bstride, rstride):
    m = np.arange(M, dtype=np.int64)
    return off + (m // rpb) * bstride + (m % rpb) * rstride


def gather_rows(buf, M, K, off, rpb, bstride, rstride, slack=128):
    """[M][K] operand rows of a flat buffer; reads behind its end see zeros (the allocation's zeroed slack)."""
    b = np.concatenate([np.asarray(buf).ravel(), np.zeros(slack, np.asarray(buf).dtype)])
    idx = row_offsets(M, off, rpb, bstride, rstride)[:, None] + np.arange(K, dtype=np.int64)[None, :]
    assert idx.max() < b.size
    return b[idx]


def gelu(x):
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    return (0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))).numpy()


class Geom:
    """The fields of wmdbg_gemm_map (include/whisper_mi355x_debug.h)."""
    FIELDS = ("M", "N", "K", "epi", "a_off", "a_rpb", "a_bstride", "a_rstride", "a_elems", "c_off", "c_rpb", "c_bstride",
              "c_rstride", "c_elems", "d_model", "n_head", "seq", "seq_pad", "batch", "vt_elems")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, int(kw.pop(f, 0)))
        assert not kw, kw

    def copy(self, **kw):
        d = {f: getattr(self, f) for f in self.FIELDS}
        d.update(kw)
        return Geom(**d)

    def __repr__(self):
        return "Geom(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS if getattr(self, f))


def plain(M, N, K, epi):
    """Contiguous operands, rows never leave one batch (what wmdbg_gemm runs)."""
    return Geom(M=M, N=N, K=K, epi=epi, a_rpb=M + 1, a_rstride=K, a_elems=M * K, c_rpb=M + 1, c_rstride=N, c_elems=M * N)


def xkv_geom(d_model, n_head, seq, batch, K=64):
    M = batch * seq
    return plain(M, 2 * d_model, K, EPI_XKV).copy(d_model=d_model, n_head=n_head, seq=seq, batch=batch, c_rpb=0, c_rstride=0,
                                                  c_elems=2 * batch * n_head * seq * 64)


def qkv_geom(d_model, n_head, seq, batch, K=64):
    M, seq_pad = batch * seq, 64 * ((seq + 63) // 64)
    return plain(M, 3 * d_model, K, EPI_QKV_ENC).copy(d_model=d_model, n_head=n_head, seq=seq, batch=batch, seq_pad=seq_pad,
                                                      c_rstride=2 * d_model, c_elems=M * 2 * d_model,
                                                      vt_elems=batch * n_head * 64 * seq_pad)


def batched_c(g, c_rpb, c_rstride=None):
    """C rows in batches of c_rpb with one guard row in front of each batch (as conv1 writes h1p)."""
    rs = g.N if c_rstride is None else c_rstride
    nb = (g.M + c_rpb - 1) // c_rpb
    return g.copy(c_off=rs, c_rpb=c_rpb, c_rstride=rs, c_bstride=(c_rpb + 1) * rs, c_elems=nb * (c_rpb + 1) * rs)


def conv1_a(g, C, T, batch):
    """A rows as conv1 reads them: [batch][T + 2][C] time-major, the window of frame t = rows t .. t + 2 (K = pad64(3 C))."""
    assert g.M == batch * T and g.K == (3 * C + 63) // 64 * 64
    return g.copy(a_off=0, a_rpb=T, a_bstride=(T + 2) * C, a_rstride=C, a_elems=batch * (T + 2) * C)


def conv2_a(g, d, S, batch):
    """A rows as conv2 reads them: [batch][2 S + 1][d] (row 0 the zero pad), frame s = rows 2 s .. 2 s + 2 (K = 3 d)."""
    assert g.M == batch * S and g.K == 3 * d
    return g.copy(a_off=0, a_rpb=S, a_bstride=(2 * S + 1) * d, a_rstride=2 * d, a_elems=batch * (2 * S + 1) * d)


def dest_index(g):
    """(c_idx, vt_idx): [M][N] int64 flat destination of every output element in C / vt, -1 where it goes to the other."""
    m = np.arange(g.M, dtype=np.int64)[:, None]
    n = np.arange(g.N, dtype=np.int64)[None, :]
    none = np.full((g.M, g.N), -1, np.int64)
    if g.epi == EPI_XKV:
        d, H = g.d_model, g.n_head
        kv, hn = n // d, n % d
        h, e = hn // 64, hn % 64
        b, s = m // g.seq, m % g.seq
        return ((((kv * g.batch + b) * H + h) * g.seq + s) * 64 + e), none
    c = g.c_off + (m // g.c_rpb) * g.c_bstride + (m % g.c_rpb) * g.c_rstride + n
    if g.epi != EPI_QKV_ENC:
        return c + 0 * m, none
    d, H = g.d_model, g.n_head
    hn = n - 2 * d
    h, e = hn // 64, hn % 64
    b, s = m // g.seq, m % g.seq
    v = ((b * H + h) * 64 + e) * g.seq_pad + vt_pos(s)
    isv = (n >= 2 * d) & (m >= 0)
    return np.where(isv, -1, c), np.where(isv, v, -1)


def values(g, A_buf, W, bias, pos=None, C0=None):
    """float64 [M][N] value of every output element before the output rounding, and the bound's S = |A| |W|^T + |bias|.
    A_buf / W are the bf16-rounded operands.  Epilogue 2 adds the element's old value C0 (flat [c_elems])."""
    A = gather_rows(A_buf, g.M, g.K, g.a_off, g.a_rpb, g.a_bstride, g.a_rstride).astype(np.float64)
    Wd = np.asarray(W, dtype=np.float64).reshape(g.N, g.K)
    bd = np.zeros(g.N) if bias is None else np.asarray(bias, dtype=np.float64)
    lin = A @ Wd.T + bd
    S = np.abs(A) @ np.abs(Wd).T + np.abs(bd)
    if g.epi in GELU_EPI:
        lin = gelu(lin)
    if g.epi == EPI_CONV2_F32:
        lin = lin + np.asarray(pos, dtype=np.float64).reshape(-1, g.N)[np.arange(g.M) % g.c_rpb]
    if g.epi == EPI_RESID_F32:
        lin = lin + np.asarray(C0, dtype=np.float64).ravel()[dest_index(g)[0]]
    return lin, S


def exact_outputs(g, vals, C0=None):
    """What the kernel must leave, bit for bit, when every value is exactly representable: (C bits, vt bits) as uint32 views
    of the widened f32 buffers, sentinels where nothing is written (EPI_RESID_F32: the old contents C0)."""
    ci, vi = dest_index(g)
    out = np.asarray(vals, dtype=np.float32)
    if g.epi == EPI_QKV_ENC:
        q = np.arange(g.N)[None, :] < g.d_model
        out = np.where(q, out * QSCALE, out).astype(np.float32)     # one f32 multiply, then the one bf16 rounding
    if g.epi in BF16_OUT:
        out = bf16(out)
    C = np.full(g.c_elems, SENT_BF16 if g.epi in BF16_OUT else SENT_F32, np.uint32)
    if g.epi == EPI_RESID_F32:
        C = np.asarray(C0, dtype=np.float32).ravel().view(np.uint32).copy()
    C[ci[ci >= 0]] = out[ci >= 0].view(np.uint32)
    vt = np.full(g.vt_elems, SENT_BF16, np.uint32)
    vt[vi[vi >= 0]] = out[vi >= 0].view(np.uint32)
    return C, vt


def bound(g, ref, S):
    """Per-element error bound of the module docstring; ref = the float64 value (EPI_QKV_ENC: before the query scale)."""
    delta = 2.0 * g.K * U * S
    if g.epi in GELU_EPI:
        delta = 1.13 * delta + 1e-6          # GELU's Lipschitz constant; twice the 4.3e-7 of gelu_erf's own comment
    if g.epi in BF16_OUT:
        return delta + 2.0 ** -8 * (np.abs(ref) + delta)
    return delta + U * np.abs(ref)


def scatter_check(g, got_C, got_vt, ref, S):
    """got_* = the hook's widened f32 buffers.  Every element: written ones within bound(), all others still the sentinel.
    Returns the largest error / bound."""
    ci, vi = dest_index(g)
    ref = np.asarray(ref, dtype=np.float64)
    bnd = bound(g, ref, S)
    if g.epi == EPI_QKV_ENC:
        q = np.arange(g.N)[None, :] < g.d_model
        ref = np.where(q, ref * float(QSCALE), ref)
        bnd = np.where(q, bnd * float(QSCALE), bnd)   # (the f32 multiply's own rounding, 2^-24 relative, is inside delta's factor 2)
    worst = 0.0
    for idx, got, sent in ((ci, got_C, SENT_BF16 if g.epi in BF16_OUT else SENT_F32), (vi, got_vt, SENT_BF16)):
        if got is None:
            assert not (idx >= 0).any()
            continue
        got = np.asarray(got, dtype=np.float32).ravel()
        w = idx >= 0
        written = np.zeros(got.size, bool)
        written[idx[w]] = True
        assert int(written.sum()) == int(w.sum()), "two outputs share a destination"
        if g.epi != EPI_RESID_F32:
            assert np.array_equal(got.view(np.uint32)[~written], np.full(int((~written).sum()), sent, np.uint32)), \
                "an element the kernel must not write lost its sentinel"
        err = np.abs(got[idx[w]].astype(np.float64) - ref[w])
        ratio = err / bnd[w]
        assert np.isfinite(ratio).all(), "non-finite output (an unwritten element?)"
        worst = max(worst, float(ratio.max()))
    return worst


# ---- operands of the exact tests: every sum is an integer of magnitude <= 256 --------------------------------------------
def exact_weights(N, K, k_used=None):
    """Small integers that change with every step in n and in k (167 is prime); columns >= k_used are zero (conv1's pad)."""
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    w = ((31 * n + 17 * k) % 167 - 83).astype(np.float32)
    if k_used is not None:
        w[:, k_used:] = 0
    return w


def exact_bias(N):
    return ((np.arange(N) % 15) - 7).astype(np.float32)


def one_hot_rows(rows, width, live=None):
    """[rows][width] with one 1 per row at a column that walks with the row; rows where live is False are zero."""
    a = np.zeros((rows, width), np.float32)
    r = np.arange(rows)
    a[r, (5 * r + 3) % width] = 1
    if live is not None:
        a[~np.asarray(live)] = 0
    return a


# ---- the conv stem -------------------------------------------------------------------------------------------------------
def conv1_ref(mel, w1, b1):
    """mel [B][C][T] -> gelu(conv1d(k 3, pad 1)) time-major [B][T][O], float64; and S of the error bound."""
    x, w, b = (torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (mel, w1, b1))
    lin = torch.nn.functional.conv1d(x, w, b, padding=1)
    S = torch.nn.functional.conv1d(x.abs(), w.abs(), b.abs(), padding=1)
    return gelu(lin.numpy()).transpose(0, 2, 1), S.numpy().transpose(0, 2, 1)


def conv2_ref(h1, w2, b2, pos):
    """h1 time-major [B][T][d] -> gelu(conv1d(k 3, stride 2, pad 1)) + pos, [B][T / 2][O], float64; and S."""
    x = torch.as_tensor(np.asarray(h1, dtype=np.float64)).permute(0, 2, 1)
    w, b = (torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (w2, b2))
    lin = torch.nn.functional.conv1d(x, w, b, stride=2, padding=1)
    S = torch.nn.functional.conv1d(x.abs(), w.abs(), b.abs(), stride=2, padding=1)
    return gelu(lin.numpy()).transpose(0, 2, 1) + np.asarray(pos, dtype=np.float64)[None], S.numpy().transpose(0, 2, 1)


def pack_conv_weight(w, kpad=None):
    """[O][C][3] -> [O][kpad], k = tap * C + c, zero columns behind 3 C."""
    O, C, _ = w.shape
    kpad = 3 * C if kpad is None else kpad
    out = np.zeros((O, kpad), w.dtype)
    out[:, :3 * C] = w.transpose(0, 2, 1).reshape(O, 3 * C)
    return out


def time_major(mel, back_pad=True):
    """[B][C][T] -> [B][1 + T (+ 1)][C] with a zero row in front (and behind)."""
    B, C, T = mel.shape
    out = np.zeros((B, T + (2 if back_pad else 1), C), mel.dtype)
    out[:, 1:T + 1] = mel.transpose(0, 2, 1)
    return out


def mel_window(block, seek, n, frames=N_FRAMES):
    """Frames seek .. seek + n - 1 of a [C][T] block, zeros from n to `frames`."""
    out = np.zeros((block.shape[0], frames), block.dtype)
    out[:, :n] = block[:, seek:seek + n]
    return out


# ---- the shapes: the smallest at which each path of the kernels can go wrong ---------------------------------------------
DH = ((64, 1), (128, 2))
XKV_SEQ = (5, 8, 9, 20, 37, 100)       # 5: below 8, the unstaged path; 8: the staged path's edge; small: several wraps per 64 rows
QKV_SEQ = (16, 20, 36, 37, 100)        # 37: later chunks start at sq % 4 != 0, the per-element V^T path
C_RPB = (5, 8, 9, 50)                  # 5: unstaged; a guard row per batch
C_N = (64, 80, 128)                    # 80: not a multiple of 64, the unstaged path
C_M = (150, 350)                       # tails against 64, 128 and 256
K_SMALL = 128                          # two K tiles: the smallest the 256 tile runs


def _conv_cases(epi1, epi2):
    out = []
    for batch in (1, 3):
        for C in (80, 128):            # 80: K = 256 over-reads 16 elements into the next row, the next batch and the slack
            T, N = 100, 64
            g = R_conv1(C, T, batch, N, epi1)
            out.append(("conv1a-C%d-T%d-B%d-e%d" % (C, T, batch, epi1), g))
        d, S, N = 64, 50, 64
        out.append(("conv2a-d%d-S%d-B%d-e%d" % (d, S, batch, epi2), R_conv2(d, S, batch, N, epi2)))
    return out


def R_conv1(C, T, batch, N, epi):
    """conv1 as the product launches it: A windows of a [batch][T + 2][C] buffer, C rows behind a guard row per batch."""
    K = (3 * C + 63) // 64 * 64
    return conv1_a(batched_c(plain(batch * T, N, K, epi), T), C, T, batch)


def R_conv2(d, S, batch, N, epi):
    """conv2 as the product launches it: A windows at stride 2 d of a [batch][2 S + 1][d] buffer, C [batch][S][N], pos [S][N]."""
    g = conv2_a(plain(batch * S, N, 3 * d, epi), d, S, batch)
    return g.copy(c_rpb=S, c_bstride=S * N)


def _scatter_cases():
    out = []
    for d, H in DH:
        for batch in (1, 3):
            for seq in XKV_SEQ:
                out.append(("xkv-d%d-s%d-B%d" % (d, seq, batch), xkv_geom(d, H, seq, batch, K_SMALL)))
            for seq in QKV_SEQ:
                out.append(("qkv-d%d-s%d-B%d" % (d, seq, batch), qkv_geom(d, H, seq, batch, K_SMALL)))
    # query | key rows behind a guard row per 5 rows: fewer than 8 rows per batch, the unstaged path scales the queries itself
    out.append(("qkv-d128-s37-B3-r5", batched_c(qkv_geom(128, 2, 37, 3, K_SMALL), 5, c_rstride=256)))
    return out


def _batched_c_cases(epis):
    return [("cmap-e%d-r%d-N%d-M%d" % (epi, rpb, N, M), batched_c(plain(M, N, K_SMALL, epi), rpb))
            for epi in epis for rpb in C_RPB for N in C_N for M in C_M]


def exact_cases():
    """(id, Geom) of the exact-placement tests: every epilogue without a GELU."""
    return (_scatter_cases() + _batched_c_cases((EPI_BIAS_BF16, EPI_F32, EPI_RESID_F32)) +
            _conv_cases(EPI_BIAS_BF16, EPI_F32) + _conv_cases(EPI_F32, EPI_BIAS_BF16))


def numeric_cases():
    """(id, Geom) of the per-element numeric tests: the same shapes with all seven epilogues, and K = 1280."""
    big = [("k1280-e%d" % e, batched_c(plain(150, 128, 1280, e), 50)) for e in (EPI_F32, EPI_GELU_BF16, EPI_RESID_F32)]
    big += [("k1280-qkv", qkv_geom(128, 2, 37, 3, 1280)), ("k1280-xkv", xkv_geom(128, 2, 37, 3, 1280)),
            ("k1280-conv2", plain(150, 128, 1280, EPI_CONV2_F32).copy(c_rpb=50, c_bstride=50 * 128))]
    return (_scatter_cases() + _batched_c_cases(range(0, 4)) + _batched_c_cases((EPI_F32,)) +
            _conv_cases(EPI_GELU_BF16, EPI_CONV2_F32) + big)


def _a_layout(g):
    """(rows, width, guard) of the A buffer: conv1-like [batch][T + 2][C], conv2-like [batch][2 S + 1][d] or plain [M][K]."""
    if g.a_bstride == (g.a_rpb + 2) * g.a_rstride:
        rows = g.a_elems // g.a_rstride
        r = np.arange(rows) % (g.a_rpb + 2)
        return rows, g.a_rstride, (r == 0) | (r == g.a_rpb + 1)
    if g.a_rstride % 2 == 0 and g.a_bstride == (2 * g.a_rpb + 1) * (g.a_rstride // 2):
        w = g.a_rstride // 2
        rows = g.a_elems // w
        return rows, w, (np.arange(rows) % (2 * g.a_rpb + 1)) == 0
    assert g.a_rstride == g.K and g.a_elems == g.M * g.K
    return g.M, g.K, np.zeros(g.M, bool)


def exact_operands(g):
    """(A flat, W [N][K], bias, C0 or None): one 1 per A buffer row (a conv window sums three weights), integer weights and
    bias; |sum| <= 3 * 83 + 7 = 256.  Guard rows are zero, as the product keeps them."""
    rows, width, guard = _a_layout(g)
    A = np.zeros(g.a_elems, np.float32)
    A[:rows * width] = one_hot_rows(rows, width, live=~guard).ravel()
    W = exact_weights(g.N, g.K, k_used=min(g.K, 3 * width) if width != g.K else None)
    C0 = None
    if g.epi == EPI_RESID_F32:
        C0 = ((np.arange(g.c_elems) * 7) % 201 - 100).astype(np.float32)
    return A, W, exact_bias(g.N), C0


def random_operands(g, seed):
    """Asymmetric random operands rounded to bf16 (a transposed or shifted fragment must show); conv1's pad columns of W are
    zero; pos[r][n] = 1000 r + n, so a wrong positional row is off by >= 1000."""
    rng = np.random.default_rng(seed)
    rows, width, _ = _a_layout(g)
    A = bf16(rng.standard_normal(g.a_elems) + np.linspace(-0.5, 0.5, g.a_elems))
    W = bf16(rng.standard_normal((g.N, g.K)) * 0.1 + np.linspace(-0.05, 0.05, g.N)[:, None])
    if width != g.K:
        W[:, 3 * width:] = 0
    bias = rng.standard_normal(g.N).astype(np.float32)
    pos = C0 = None
    if g.epi == EPI_CONV2_F32:
        pos = (1000.0 * np.arange(g.c_rpb)[:, None] + np.arange(g.N)[None, :]).astype(np.float32)
    if g.epi == EPI_RESID_F32:
        C0 = rng.standard_normal(g.c_elems).astype(np.float32)
    return A, W, bias, pos, C0
