"""float64 numpy restatement of layernorm_kernel (csrc/enc_kernels.hip), a per-element error bound derived from the kernel's own
order of operations, an f32 emulation of that order (with the value-only mistakes the bound must catch), and the inputs of the
GPU tests.  Shared by test_layernorm_ref_cpu.py, test_layernorm_kernel_gpu.py and test_encoder_stages_gpu.py.  Nothing here is
imported from the package.

Restatement      y = (x - mean) / sqrt(var + 1e-5) * g + b over the last axis, var = the mean of (x - mean)^2 (divisor d).

The kernel       One wave of 64 lanes per row.  MAXP = 1 (d <= 256), 3 (d <= 768) or 5 (d <= 1280) quads of four columns per lane,
                 quad i of lane L = columns 4 (64 i + L) .. + 3, zeros behind the row.  s = the lane's sum of (x + y) + (z + w)
                 over its quads, a 6-step butterfly over the lanes, mean = s / d; then the centred second pass a = x - mean,
                 (a^2 + c^2) + (e^2 + f^2) per quad, the same butterfly, rstd = rsqrtf(q / d + 1e-5); y = a * rstd * g + b.

Bound            v = 2^-24.  An element passes through n = MAXP + 2 + 6 f32 additions on its way into s (two inside its quad, at
                 most MAXP along the lane, six in the butterfly), so |s - sum x| <= n v sum |x|; the division adds at most 2 v
                 |mean| (v when it is correctly rounded).  With Xbar = sum |x| / d:
                     dm = (n + 2) v Xbar                  -- the mean's error: it scales with sum |x| / d, not with the spread
                 a = fl(x - mean^) = (c - dm')(1 + v), c = x - mean, |dm'| <= dm.  sum (c - dm')^2 = d (var + dm'^2): the cross
                 term vanishes.  Each a^2 carries 3 v (a twice, the square), the sum n v, q / d and + eps one v each:
                     rho = (n + 5) v + dm^2 / (var + eps) -- relative error of var^ + eps
                 rsqrtf is one ulp (2 v): rstd^ = rstd (1 + rho / 2 + 2 v).  y^ = fl(fl(fl(a rstd^) g) + b): a's own v and the
                 two products' 2 v on top, v |y| for the last addition (a fused multiply-add only removes a rounding):
                     bound = rstd |g| (dm + (|c| + dm)(rho / 2 + 5 v)) + v |y|
                 First order in v throughout; the second-order terms are below v^2 n^2 of the first and not carried.
                 The bf16 output is RNE of the same f32 value the kernel stores to the f32 output: bit-equal, no bound."""
import numpy as np

V = 2.0 ** -24
EPS = 1e-5
MUTANTS = ("one_pass", "eps_1e-6", "divisor_d-1", "last_quad_dropped", "reads_one_quad_more")
DS = (4, 64, 252, 256, 260, 384, 764, 768, 772, 1024, 1276, 1280)
ROWS = (1, 2, 3, 4, 5, 9)
KINDS = ("normal", "mean30", "outlier", "constant")


def bf16(x):
    """float -> nearest-even bf16, returned as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def maxp(d):
    assert d % 4 == 0 and 4 <= d <= 1280
    return 1 if d <= 256 else 3 if d <= 768 else 5


def restate(x, g, b, eps=EPS):
    """-> (y, bound), float64 [rows][d]"""
    x, g, b = (np.asarray(a, dtype=np.float64) for a in (x, g, b))
    d = x.shape[-1]
    n = maxp(d) + 2 + 6
    mean = x.mean(axis=-1, keepdims=True)
    c = x - mean
    var = (c * c).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = c * rstd * g + b
    dm = (n + 2) * V * np.abs(x).mean(axis=-1, keepdims=True)
    rho = (n + 5) * V + dm * dm / (var + eps)
    bound = rstd * np.abs(g) * (dm + (np.abs(c) + dm) * (rho / 2 + 5 * V)) + V * np.abs(y)
    return y, bound


def _butterfly(s):
    f = np.float32
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lane ^ o]).astype(f)
    return s


def emulate(x, g, b, mutant=None):
    """f32, in the kernel's order.  -> y f32 [rows][d].  mutant: one of MUTANTS -- the variance as E[x^2] - mean^2 in one pass;
    eps 1e-6; the divisor d - 1; the row's last quad left out of the sums and the output (it stays zero); the row read with
    `idx <= np`: one quad more, the next row's first (the last row reads zeros), in both sums."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    x, g, b = (np.ascontiguousarray(a, dtype=f) for a in (x, g, b))
    rows, d = x.shape
    P, npq = maxp(d), d // 4
    live = npq - 1 if mutant == "last_quad_dropped" else npq
    xp = np.zeros((rows, P * 64 * 4 + 4), f)
    xp[:, :d] = x
    if mutant == "reads_one_quad_more":
        xp[:-1, d:d + 4] = x[1:, :4]
        live = npq + 1
    xq = xp[:, :P * 256].reshape(rows, P, 64, 4)            # [row][i][lane][component]: quad idx = i * 64 + lane
    if mutant == "reads_one_quad_more" and npq == P * 64:
        live = npq                                             # (the register file has no slot for it: this d cannot show it)
    idx = np.arange(P)[:, None] * 64 + np.arange(64)[None, :]
    on = (idx < live)[None, :, :, None]
    v = np.where(on, xq, f(0))
    s = np.zeros((rows, 64), f)
    for i in range(P):
        s = (s + ((v[:, i, :, 0] + v[:, i, :, 1]).astype(f) + (v[:, i, :, 2] + v[:, i, :, 3]).astype(f)).astype(f)).astype(f)
    mean = (_butterfly(s) / f(d)).astype(f)                    # every lane holds the same value
    q = np.zeros((rows, 64), f)
    for i in range(P):
        a = (v[:, i] - (f(0) if mutant == "one_pass" else mean[:, :, None])).astype(f)
        a = np.where(on[:, i], a, f(0))
        sq = (a * a).astype(f)
        q = (q + ((sq[..., 0] + sq[..., 1]).astype(f) + (sq[..., 2] + sq[..., 3]).astype(f)).astype(f)).astype(f)
    q = _butterfly(q)
    div = f(d - 1) if mutant == "divisor_d-1" else f(d)
    var = (q / div).astype(f)
    if mutant == "one_pass":
        var = (var - (mean * mean).astype(f)).astype(f)
    eps = f(1e-6) if mutant == "eps_1e-6" else f(EPS)
    rstd = (1.0 / np.sqrt((var + eps).astype(f).astype(np.float64))).astype(f)[:, 0]
    m = mean[:, 0]
    y = ((((x - m[:, None]).astype(f) * rstd[:, None]).astype(f) * g).astype(f) + b).astype(f)
    if mutant == "last_quad_dropped":
        y[:, d - 4:] = 0
    return y


def params(d):
    """asymmetric g and b: a column shifted by one shows"""
    rng = np.random.default_rng(7000 + d)
    g = (1 + 0.3 * rng.standard_normal(d) + np.linspace(-0.3, 0.3, d)).astype(np.float32)
    b = (0.5 * rng.standard_normal(d) + np.linspace(0.5, -0.5, d)).astype(np.float32)
    return g, b


def inputs(rows, d, kind):
    """x f32 [rows][d].  normal: row r at scale 3, 0.3 or 0.03 (r % 3) around 1.5 x its scale, so that eps is seen at the small
    ones; mean30: mean = 30 x the standard deviation; outlier: one column per row at 1e4 x the rest, as Whisper's residual
    stream has; constant: every row one value (variance 0: y = b)."""
    rng = np.random.default_rng(100000 * KINDS.index(kind) + 1300 * rows + d)
    z = rng.standard_normal((rows, d))
    r = np.arange(rows)
    if kind == "normal":
        sc = np.array([3.0, 0.3, 0.03])[r % 3][:, None]
        x = (z + 1.5) * sc
    elif kind == "mean30":
        x = z + 30.0
    elif kind == "outlier":
        x = z.copy()
        x[r, (37 * r + 3) % d] = 1e4 * (1 + 0.1 * r)
    else:
        x = np.repeat((1.1 + 0.7 * r)[:, None], d, axis=1) * np.where(r % 2 == 0, 1.0, -1.0)[:, None]
    return x.astype(np.float32)


def cases():
    """(rows, d): every instantiation boundary x every row tail, and the encoder's own launch shape at d = 384"""
    return [(rows, d) for d in DS for rows in ROWS] + [(1500, 384)]


def bf16_bracket(y, bound):
    """(lo, hi) f32: a launch that writes only the bf16 output must leave RNE of an f32 value within y +- bound, i.e. lo <= out <=
    hi (rounding is monotone; the f64 -> f32 step is widened by one f32 ulp outwards)"""
    lo = np.nextafter((np.asarray(y) - bound).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter((np.asarray(y) + bound).astype(np.float32), np.float32(np.inf))
    return bf16(lo), bf16(hi)
