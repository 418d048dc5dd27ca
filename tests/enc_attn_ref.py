"""float64 numpy restatement of the encoder attention (enc_attn_kernel of csrc/enc_kernels.hip), a per-element error bound derived
from the kernel's rounding points, an emulation of the kernel's order of operations (with the value-only mistakes the bound must
catch), and the builders of the exact probes.  Shared by test_enc_attn_ref_cpu.py, which holds this module to its conditions,
and the GPU tests test_enc_attention_kernels_gpu.py / test_encoder_stages_gpu.py.  Nothing here is imported from the package.

Restatement      q, k, v f32 [B][S][H * 64], k and v bf16-exact.  The kernel receives qs = bf16(f32(q) * QSCALE), QSCALE =
                 0.125 * log2(e) as the f32 product model.h writes.  Scores s[i][j] = sum_e qs[i][e] k[j][e] are in log2 units,
                 w = softmax2(s) over the S keys of the (chunk, head) pair, ref = w v, A = w |v|.

The kernel       64-key tiles.  r = the first tile's maximum; later r moves (by delta = max(m, 0) per query, m = the tile's largest
                 s - r) iff ANY of the 32 queries of the wave has m > 8, and O, l are multiplied by alpha = exp2(-delta).
                 p = exp2(s - r) in f32; P = bf16(p) feeds O += P v; l += p (f32 adds) -- or, in the SUM_MFMA variant, l += P.
                 out = bf16(O / l).

Bound            u = 2^-8 (bf16 unit roundoff), v = 2^-24 (f32).  Write p_j (1 + e_j) for the f32 value the kernel holds for key j
                 relative to the final r, T_j = sum_e |qs_e| |k_je|, R = max_j |s_j| (|r| <= R: r is a sum of score differences
                 that ends at a score).
                   * the score chain: 64 products (exact in f32) and the C operand -r summed by the matrix pipe, then at most one
                     subtraction of delta: |d(s_j - r)| <= 2 (64 + 2) v (T_j + R), the factor 2 as in enc_gemm_ref (the pipe's
                     internal rounding is not documented as round-to-nearest per step); r += delta is one more f32 rounding of a
                     number <= R, inside the same term.  Through exp2 this is a relative ln2 * 2 * 66 v (T_j + R);
                   * v_exp_f32: one ulp, 2 v relative;
                   * alpha: one ulp of v_exp_f32 and one rounding of the product per move, on O and on l; the two copies of
                     alpha's own error cancel in O / l only for keys of earlier tiles, not against later ones: 4 v per move,
                     at most ntiles - 1 moves.
                   E_j = ln2 * 132 v (T_j + R) + 2 v + 4 v (ntiles - 1).
                   * O and l are f32 sums of S terms: 2 S v (A + |ref|), any order, the factor 2 as above;
                   * 1 / l and the product with it: 4 v |ref|.
                   f32 terms = sum_j w_j E_j (|v_j| + |ref|) + 2 S v (A + |ref|) + 4 v |ref|.
                   * P = bf16(p) with l summing the unrounded p: out - ref gains sum_j (P_j - p_j) v_j / l, <= u A.
                     SUM_MFMA (l sums the rounded P): sum_j (P_j - p_j)(v_j - ref) / l, <= u (A + |ref|);
                   * the output rounding: u |ref| (first order; the second-order u * error is inside the factor 2 slack).
                 bound = u (A + |ref|) + f32 terms,  SUM_MFMA: u (A + 2 |ref|) + f32 terms.
                 Denormal p (s - r < -126) are flushed: an absolute 2^-126 S, not carried.

Exact probes     One-hot queries (after the pre-scale) against keys that carry small integers in that dimension: every score is
                 an integer, every p a power of two, column c of the one-hot V reads w[i][mark[c]] = 2^s / sum 2^s.  The gate is
                 half a bf16 ulp of that value plus the f32 terms that remain: v_exp_f32 is specified to one ulp, not as exact
                 at integers, so p and alpha keep 2 v and 3 v per move; l is an f32 sum of S terms (S v, exact while < 2^24 but
                 not at an excess of 40); 1 / l and the product 3 v.  O has one non-zero product per column: no sum."""
import numpy as np

U = 2.0 ** -8
V = 2.0 ** -24
LN2 = float(np.log(2.0))
QSCALE = np.float32(0.125) * np.float32(1.44269504088896340736)
THR = 8.0
MUTANTS = ("drop_last", "double_key", "alpha_half", "alpha_half_acc", "per_lane_stale_c", "sum_rounded")


def bf16(x):
    """float -> nearest-even bf16, returned as float32 (NaN stays NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_ulp(x):
    """the spacing of bf16 at |x|; 0 at 0"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(a > 0, 2.0 ** (np.floor(np.log2(np.where(a > 0, a, 1.0))) - 7), 0.0)


def prescale(q):
    """q f32 as the kernel receives it"""
    return bf16(np.asarray(q, dtype=np.float32) * QSCALE)


def heads(a, H):
    """[B][S][H * 64] -> float64 [B][H][S][64]"""
    B, S, d = a.shape
    assert d == H * 64
    return np.asarray(a, dtype=np.float64).reshape(B, S, H, 64).transpose(0, 2, 1, 3)


def unheads(a):
    """[B][H][S][64] -> [B][S][H * 64]"""
    B, H, S, _ = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(B, S, H * 64)


class Ref:
    """ref, A and the two bounds, each [B][S][H * 64] float64"""


def restate(q, k, v, H, qs=None):
    """The restatement and its bounds.  qs: the pre-scaled queries when they are already given (the product's m->qk)."""
    qh = heads(prescale(q) if qs is None else qs, H)
    kh, vh = heads(k, H), heads(v, H)
    B, _, S, _ = qh.shape
    nt = (S + 63) // 64
    ref, A, f32 = (np.zeros((B, H, S, 64)) for _ in range(3))
    for b in range(B):
        for h in range(H):
            s = qh[b, h] @ kh[b, h].T
            T = np.abs(qh[b, h]) @ np.abs(kh[b, h]).T
            R = np.abs(s).max(axis=1, keepdims=True)
            w = np.exp2(s - s.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            av = np.abs(vh[b, h])
            ref[b, h] = w @ vh[b, h]
            A[b, h] = w @ av
            E = LN2 * 132 * V * (T + R) + 2 * V + 4 * V * (nt - 1)
            wE = w * E
            f32[b, h] = wE @ av + wE.sum(axis=1, keepdims=True) * np.abs(ref[b, h])
    r = Ref()
    r.ref, r.A = unheads(ref), unheads(A)
    r.f32 = unheads(f32) + 2 * S * V * (r.A + np.abs(r.ref)) + 4 * V * np.abs(r.ref)
    r.bound = (U * (r.A + np.abs(r.ref)) + r.f32, U * (r.A + 2 * np.abs(r.ref)) + r.f32)   # [enc_attn_mfma_sum]
    return r


def triple_loop(q, k, v, H):
    """(ref, A) by loops over query, key and dimension: what restate() must equal"""
    B, S, d = q.shape
    qs = prescale(q).astype(np.float64)
    ref, A = np.zeros((B, S, d)), np.zeros((B, S, d))
    for b in range(B):
        for h in range(H):
            c = slice(h * 64, h * 64 + 64)
            for i in range(S):
                s = [sum(qs[b, i, h * 64 + e] * float(k[b, j, h * 64 + e]) for e in range(64)) for j in range(S)]
                m = max(s)
                p = [2.0 ** (x - m) for x in s]
                den = sum(p)
                for j in range(S):
                    ref[b, i, c] += p[j] / den * v[b, j, c].astype(np.float64)
                    A[b, i, c] += p[j] / den * np.abs(v[b, j, c].astype(np.float64))
    return ref, A


# ---- the kernel's order --------------------------------------------------------------------------------------------------
def _emulate_pair(qs, k, v, sum_rounded, mutant, double_key):
    S = qs.shape[0]
    nt = (S + 63) // 64
    kp, vp = np.zeros((nt * 64, 64)), np.zeros((nt * 64, 64))
    kp[:S], vp[:S] = k, v
    f = np.float32
    ref, cref, l = np.zeros(S, f), np.zeros(S, f), np.zeros(S, f)
    O = np.zeros((S, 64), f)
    live = S - 1 if mutant == "drop_last" else S
    wave = np.arange(S) // 32                      # 32 consecutive queries share a wave (rows behind S repeat row S - 1)
    moves = 0
    for j in range(nt):
        acc = (qs @ kp[j * 64:j * 64 + 64].T - cref[:, None].astype(np.float64)).astype(f)
        acc[:, j * 64 + np.arange(64) >= live] = f(-1e30)
        m = acc.max(axis=1)
        if j == 0:
            move, delta = np.ones(S, bool), m
        else:
            over = m > f(THR)
            move = over if mutant == "per_lane_stale_c" else (np.bincount(wave, over) > 0)[wave]
            delta = np.where(move, np.maximum(m, f(0)), f(0)).astype(f)
            moves += int((delta > 0).sum())
        ref = (ref + delta).astype(f)
        acc = (acc - delta[:, None]).astype(f)
        if j > 0:
            alpha = np.exp2(-(delta.astype(np.float64) / (2.0 if mutant == "alpha_half" else 1.0))).astype(f)
            ncol = 32 if mutant == "alpha_half_acc" else 64
            O[:, :ncol] = (O[:, :ncol] * alpha[:, None]).astype(f)
            l = (l * alpha).astype(f)
        if j == 0 or mutant != "per_lane_stale_c":
            cref = ref.copy()
        p = np.exp2(acc.astype(np.float64)).astype(f)
        if mutant == "double_key" and j * 64 <= double_key < j * 64 + 64:
            p[:, double_key - j * 64] *= f(2)
        P = bf16(p)
        l = (l + (P if (sum_rounded or mutant == "sum_rounded") else p).astype(np.float64).sum(axis=1)).astype(f)
        O = (O + P.astype(np.float64) @ vp[j * 64:j * 64 + 64]).astype(f)
    inv = (f(1) / l).astype(f)
    return bf16((O * inv[:, None]).astype(f)), moves


def emulate(q, k, v, H, sum_rounded=False, mutant=None):
    """-> (out f32 [B][S][H * 64] holding bf16 values, the number of (query, tile) moves after the first tile).  mutant: one of
    MUTANTS -- the last key dropped; key S // 2 counted twice; alpha = 2^(-delta / 2); alpha on the first 32 output columns
    only; the move decided per lane with the C operand left at the first tile's reference; l from the rounded P."""
    assert mutant is None or mutant in MUTANTS
    qh, kh, vh = heads(prescale(q), H), heads(k, H), heads(v, H)
    B, _, S, _ = qh.shape
    out = np.zeros((B, H, S, 64), np.float32)
    moves = 0
    for b in range(B):
        for h in range(H):
            out[b, h], n = _emulate_pair(qh[b, h], kh[b, h], vh[b, h], sum_rounded, mutant, S // 2)
            moves += n
    return unheads(out), moves


# ---- the per-element spread: inputs and cases ------------------------------------------------------------------------------
SPREAD_S = (1, 28, 63, 64, 65, 127, 128, 129, 192, 193, 1500)
SPREAD_BH = ((1, 1), (3, 2))
PEAK = 2.5


def spread_cases():
    """(B, H, S, kind): every S x (B, H) x input kind, and the one case with nine live pairs of a grid padded to sixteen"""
    out = [(B, H, S, kind) for S in SPREAD_S for B, H in SPREAD_BH for kind in ("normal", "peaked")]
    return out + [(3, 3, 129, "normal")]


def spread_inputs(B, H, S, kind):
    """bf16-exact q, k, v [B][S][H * 64]: N(0, 1), v with a ramp over the columns (a transposed head or dimension shows);
    "peaked": q x 2.5, which makes hundreds of rows take late moves of the reference."""
    rng = np.random.default_rng(1000 * S + 10 * B + H)
    d = H * 64
    q = rng.standard_normal((B, S, d)) * (PEAK if kind == "peaked" else 1.0)
    k = rng.standard_normal((B, S, d))
    v = rng.standard_normal((B, S, d)) + np.linspace(-1, 1, d)[None, None, :]
    return bf16(q), bf16(k), bf16(v)


# ---- exact probes ---------------------------------------------------------------------------------------------------------
def probe_dim(h):
    """the dimension that carries head h's one-hot query"""
    return (7 + 13 * h) % 64


def default_marks(kint, pair):
    """min(S, 64) distinct keys for the 64 columns of one pair (-1: column unused): the keys that carry a non-zero integer with
    their neighbours, the first and last key and the tile edges first, then keys spread over the row, rotated by the pair."""
    S = len(kint)
    if S <= 64:
        return np.concatenate([np.roll(np.arange(S), pair), np.full(64 - S, -1)])
    first = []
    for j in np.flatnonzero(kint)[:12]:
        first += [j, j - 1, j + 1]
    first += [0, S - 1, 63, 64, S - 2, (S - 1) // 64 * 64, (S - 1) // 64 * 64 - 1]
    rest = (np.arange(S) * 997 + 131 * pair) % S                 # 997 is prime: a permutation for every S below it ...
    seen, out = set(), []
    for j in list(first) + [int(x) for x in rest] + list(range(S)):   # ... and every key still comes up for larger S
        if 0 <= j < S and j not in seen:
            seen.add(int(j))
            out.append(int(j))
        if len(out) == 64:
            break
    return np.roll(np.array(out), pair)


def threshold_probe(amp, kint, marks=None):
    """amp [B][H][S]: the bf16-exact value the pre-scaled query i must hold in its one dimension; kint [B][H][S]: the integer
    key j carries there.  -> q, k, v f32 [B][S][H * 64], exact float64 [B][S][H * 64], marks [B][H][64].
    exact[b][i][h * 64 + c] = 2^(amp_i kint_m) / sum_j 2^(amp_i kint_j), m = marks[b][h][c] (0 where the column is unused)."""
    amp, kint = np.asarray(amp, np.float64), np.asarray(kint, np.int64)
    B, H, S = amp.shape
    d = H * 64
    q, k, v = (np.zeros((B, S, d), np.float32) for _ in range(3))
    exact = np.zeros((B, S, d))
    allm = np.zeros((B, H, 64), np.int64)
    for b in range(B):
        for h in range(H):
            e0 = h * 64 + probe_dim(h)
            q[b, :, e0] = (amp[b, h] / float(QSCALE)).astype(np.float32)
            k[b, :, e0] = kint[b, h]
            mk = default_marks(kint[b, h], b * H + h) if marks is None else np.asarray(marks[b][h])
            allm[b, h] = mk
            s = amp[b, h][:, None] * kint[b, h][None, :].astype(np.float64)
            assert np.array_equal(s, np.round(s)), "a score of the probe is not an integer"
            w = np.exp2(s - s.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            for c in np.flatnonzero(mk >= 0):
                v[b, mk[c], h * 64 + c] = 1.0
                exact[b, :, h * 64 + c] = w[:, mk[c]]
    got = prescale(q)                      # the rounding the hook applies, recomputed: the one-hot holds exactly amp
    for b in range(B):
        for h in range(H):
            assert np.array_equal(got[b, :, h * 64 + probe_dim(h)].astype(np.float64), amp[b, h]), "pre-scaled query is not amp"
    return q, k, v, exact, allm


def probe_gate(exact, S):
    """per element: half a bf16 ulp of the exact value plus the f32 terms of the module docstring"""
    nt = (S + 63) // 64
    return 0.5 * bf16_ulp(exact) + (S + 2 + 3 * (nt - 1) + 3) * V * np.abs(exact)


CODE_SEED = 20240
CODE_ROWS = 1500


def code_matrix():
    """+-1 rows [1500][64] of the selection probe; test_enc_attn_ref_cpu.py holds their largest off-diagonal product"""
    return np.random.default_rng(CODE_SEED).choice(np.array([-1.0, 1.0], np.float32), size=(CODE_ROWS, 64))


def probe_values(pair, S):
    """v [S][64] = non-zero integers / 16 (bf16-exact, |v| < 8) that differ from key to key in every column and pair to pair"""
    j, e = np.arange(S)[:, None], np.arange(64)[None, :]
    mag = (j * 37 + e * 11 + pair * 53) % 127 + 1
    return (mag * np.where((j + e) % 2 == 0, 1, -1) / 16.0).astype(np.float32)


def selection_probe(B, H, S):
    """Query i of pair (b, h) selects key pi_bh(i) of a permutation that differs from pair to pair: keys 16 x code, queries the
    code rows in permuted order.  The selected key leads every other by (64 - g) * 16 * bf16(QSCALE) log2 units, g = the
    largest off-diagonal product of the code (>= 57 for g <= 44), so the output row is v[pi(i)] bit for bit.
    -> q, k, v, want [B][S][H * 64]"""
    code = code_matrix()
    d = H * 64
    q, k, v, want = (np.zeros((B, S, d), np.float32) for _ in range(4))
    for b in range(B):
        for h in range(H):
            pair = b * H + h
            pi = np.random.default_rng(S * 131 + pair).permutation(S)
            c = slice(h * 64, h * 64 + 64)
            k[b, :, c] = 16.0 * code[:S]
            q[b, :, c] = code[pi]
            v[b, :, c] = probe_values(pair, S)
            want[b, :, c] = v[b, pi, c]
    return q, k, v, want


# ---- the threshold probes' cases -----------------------------------------------------------------------------------------
EXCESS = (7, 8, 9, 12, 40)             # 7, 8: kept (p = 128, 256); 9: the smallest move; 12: old mass matters; 40: it does not
PROBE_S = (128, 200, 1500)
MIXED_AMP = (-1.0, 0.0, 0.5, 1.0, 1.125, 1.5, 2.0, 5.0)   # x key 8: excesses -8, 0, 4, 8 | 9, 12, 16, 40 in one wave


def key_positions(S):
    """a key of tile 1, of a middle tile and of the last tile (partial unless S % 64 == 0)"""
    nt = (S + 63) // 64
    return 64 + 5, min((nt // 2) * 64 + 17, S - 2), S - 3


def threshold_cases():
    """(id, amp [B][H][S], kint [B][H][S]).  Head 1 carries the same pattern one key later, so the heads differ."""
    out = []
    for S in PROBE_S:
        for e in EXCESS:                              # chunk b: the one key at the b-th position
            kint = np.zeros((3, 2, S), np.int64)
            for b, pos in enumerate(key_positions(S)):
                kint[b, 0, pos], kint[b, 1, pos + 1] = e, e
            out.append(("base-S%d-e%d" % (S, e), np.ones((3, 2, S)), kint))
    for S, pos in ((200, 150), (1500, 1490)):         # the 32 queries of a wave disagree; wave 2 (queries 64 .. 95) never moves
        amp = np.zeros((1, 2, S))
        i = np.arange(S)
        for h in range(2):
            amp[0, h] = np.array(MIXED_AMP)[(5 * i + h) % 8]
            amp[0, h, 64:96] = np.array(MIXED_AMP[:4])[(i[64:96] + h) % 4]
        kint = np.zeros((1, 2, S), np.int64)
        kint[0, 0, pos], kint[0, 1, pos + 1] = 8, 8
        out.append(("mixed-S%d" % S, amp, kint))
    for S in (200, 1500):                             # two equal maxima in different tiles
        kint = np.zeros((3, 2, S), np.int64)
        last = S - 5
        for h in range(2):
            kint[0, h, [69 + h, last + h]] = 12       # the second after the move: it meets the reference exactly
            kint[1, h, [69 + h, 140 + h]] = 6         # both before a move (kept at p = 64) ...
            kint[1, h, last + h] = 20                 # ... which a later key forces
            kint[2, h, [69 + h, last + h]] = 8        # both exactly at the threshold: never a move
        out.append(("peaks-S%d" % S, np.ones((3, 2, S)), kint))
    return out
