"""Plain-numpy restatement of the decoder's single-query attention (csrc/dec_kernels.hip: attn_load_block, attn_block,
attn_stream_reduce, attn_merge_core) and the exact-answer probes of tests/test_dec_attention_kernels_gpu.py.

ROW GEOMETRY (stated once; the kernels' comment "single-query attention" says the same).  The keys of a (sequence, head) pair
are dealt to NS streams, NS = 8 for the cross-attention and 4 for the causal self-attention.  With i the row index RELATIVE to
the pair's first key:
    stream(i)    = (i // 8) % NS          the wave that walks the row
    row_group(i) = i % 8                  the 8 lanes of the wave that hold its 128 bytes
    load(i)      = (i // (NS * 8)) % 4    load u of a block strides by NS * 8 rows
    block(i)     = i // (NS * 8 * 4)      a block is NS * 8 * 4 rows: 256 (cross), 128 (self)
A stream keeps a running (max, sum, o[64]) over its blocks in order (online softmax, one rescale per block), its 8 row groups
are summed once, and the NS partials are merged once in stream order.  boundary_keys() derives the key positions at which
one of these indices wraps.

attention_f64 is the reference: a softmax over the keys [lo, hi] in f64 on the inputs the hooks upload (K and V rounded to
bf16, the query f32).  streamed_attention is the same result computed the kernels' way, with a `fault` argument that
reproduces one known-wrong kernel at a time: tests/test_dec_attn_ref_cpu.py shows that each probe rejects the faults it is
meant for.

PROBES (builders below; every K and V element outside a pair's key range is NaN):
  counting   k = 0 in range, so every key weighs exactly 1 / n; v[j][e] = 1 for the key j marked for column e.
             out[e] = (times key j was counted) / n: one bf16 ulp around 1 / n where marked, exactly 0 elsewhere.
  selection  k[j] = 16 * code[j], q = code[j*], code a fixed +-1 matrix: score 128 against <= 72, the answer is v[j*] bit
             for bit (v = non-zero integers / 16).
  two-peak   q = code[a] + code[b]: two equal maxima; the answer is (v[a] + v[b]) / 2 bit for bit.
  spread     scores of standard deviation ~3, v of mixed sign and magnitude; the per-element gate of spread_gate().

MEASURED (this module's own checks, tests/test_dec_attn_ref_cpu.py):
  * code = default_rng(2024) +-1 [1536][64]: largest off-diagonal code . code = 36 of 64, so a selected score (128) leads every
    other by at least 56; the f64 answer of the selection probe equals v[j*] for every n_keys in 1 .. 1536 (difference 0, below
    the 3e-24 the margin promises).
  * the numpy f32 restatement with a different summation order (attention_f32_plain: one global maximum, keys summed in
    ascending order, bf16 output), worst |out - ref| / gate over 6 pairs: 0.434 (cross, 1500 keys), 0.615 (cross, 437),
    0.467 (self, 448), 0.618 (self, 37) -- most of it the half-ulp of the bf16 output, which is the gate's first term.
  * the kernels on the MI355X: 0.40 - 0.66 (cross variants), 0.53 (self), 0.57 (candidate groups), 0.62 - 0.75 (fused query).
"""
import numpy as np

NS_CROSS, NS_SELF = 8, 4
U = 4                    # loads per block
ATT_MAXK = 1536          # WM_ATT_MAXK
CODE_SEED = 2024
MIN_LEAD = 56.0          # a selected score leads every other by at least this much (exp(-56) = 4.8e-25)


def bf16(x):
    """round to nearest even to bf16, returned as f32 (what the hooks' f2bf does; NaN stays NaN)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def bf16_ulp(x):
    """the spacing of bf16 at |x| (x != 0)"""
    return 2.0 ** (np.floor(np.log2(np.abs(x))) - 7)


def stream_of(i, NS):
    return (i // 8) % NS


def block_of(i, NS):
    return i // (NS * 8 * U)


def load_of(i, NS):
    return (i // (NS * 8)) % U


def boundary_keys(n, NS):
    """the key positions (relative to the first key) at which a row group, a stream, a load or a block wraps, and the last two"""
    s, b = NS * 8, NS * 8 * U
    ks = {0, 1, 7, 8, s - 1, s, s + 1, b - 1, b, b + 1, 2 * b - 1, 2 * b, 5 * b - 1, 5 * b, n - 2, n - 1}
    return sorted(k for k in ks if 0 <= k < n)


# ------------------------------------------------------------------ the reference and the streamed restatement
def attention_f64(q, k, v, lo, hi):
    """q [64], k / v [T][64]; softmax(q . k[lo .. hi] / 8) . v[lo .. hi] in f64"""
    q = np.asarray(q, np.float64)
    kk, vv = np.asarray(k[lo:hi + 1], np.float64), np.asarray(v[lo:hi + 1], np.float64)
    s = kk @ q / 8.0
    p = np.exp(s - s.max())
    return (p @ vv) / p.sum()


def attention_rows(q, k, v, lo, hi, entry=None):
    """q [R][H * 64], k / v [E][H][T][64]; row r attends to keys [lo[r], hi[r]] of cache entry entry[r] (default r) -> f64 [R][H * 64]"""
    R, H = q.shape[0], k.shape[1]
    lo, hi = np.broadcast_to(lo, (R,)), np.broadcast_to(hi, (R,))
    out = np.zeros((R, H * 64))
    for r in range(R):
        e = r if entry is None else entry[r]
        for h in range(H):
            out[r, h * 64:(h + 1) * 64] = attention_f64(q[r, h * 64:(h + 1) * 64], k[e, h], v[e, h], int(lo[r]), int(hi[r]))
    return out


def attention_f32_plain(q, k, v, lo, hi):
    """An f32 restatement with ANOTHER summation order than the kernels': one global maximum, the keys added in ascending order
    with f32 accumulators, f32 exp, the result rounded to bf16."""
    qe = np.asarray(q, np.float32) * np.float32(0.125)
    kk, vv = np.asarray(k[lo:hi + 1], np.float32), np.asarray(v[lo:hi + 1], np.float32)
    s = np.zeros(kk.shape[0], np.float32)
    for e in range(64):
        s = s + kk[:, e] * qe[e]
    p = np.exp(s - s.max()).astype(np.float32)
    o, l = np.zeros(64, np.float32), np.float32(0)
    for j in range(kk.shape[0]):
        o = o + p[j] * vv[j]
        l = np.float32(l + p[j])
    return bf16(o / l)


FAULTS = ("drop_last_of_partial_block", "count_twice", "no_rescale", "merge_unaligned", "swap_v_rows", "read_past_end")


def streamed_attention(q, k, v, lo, hi, NS, fault=None, fault_key=None):
    """The kernels' algorithm in f64: streams, blocks of NS * 32 rows, online softmax per stream, merge in stream order.
    fault (one of FAULTS) makes it one known-wrong kernel:
      drop_last_of_partial_block  the last key is masked when the key count is no multiple of the block
      count_twice                 key fault_key (relative) is accumulated twice
      no_rescale                  the running sum and output are not rescaled when the maximum moves
      merge_unaligned             the streams' partials are added without aligning their maxima
      swap_v_rows                 V rows fault_key and fault_key ^ 1 (the same group of 8) change places
      read_past_end               the row behind the last key is taken into the softmax"""
    assert fault is None or fault in FAULTS
    q = np.asarray(q, np.float64) * 0.125
    n = hi - lo + 1
    n_eff = n
    if fault == "drop_last_of_partial_block" and n % (NS * 8 * U):
        n_eff = n - 1
    if fault == "read_past_end":
        n_eff = n + 1
    kk, vv = np.asarray(k[lo:lo + n_eff], np.float64), np.array(v[lo:lo + n_eff], np.float64)
    if fault == "swap_v_rows" and (fault_key ^ 1) < n_eff:
        vv[[fault_key, fault_key ^ 1]] = vv[[fault_key ^ 1, fault_key]]
    m, l, o = np.full(NS, -1e30), np.zeros(NS), np.zeros((NS, 64))
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(NS):
            for r0 in range(0, n_eff, NS * 8 * U):
                rows = [r0 + u * NS * 8 + w * 8 + rg for u in range(U) for rg in range(8)]
                rows = [i for i in rows if i < n_eff]
                sc = kk[rows] @ q if rows else np.zeros(0)
                m_new = max(m[w], sc.max()) if rows else m[w]
                resc = 1.0 if fault == "no_rescale" and m[w] > -1e29 else np.exp(m[w] - m_new)
                l[w] *= resc
                o[w] *= resc
                p = np.exp(sc - m_new)
                if fault == "count_twice":
                    p = p * np.array([2.0 if i == fault_key else 1.0 for i in rows])
                l[w] += p.sum()
                if rows:
                    o[w] += p @ vv[rows]
                m[w] = m_new
        if fault == "merge_unaligned":
            return o.sum(axis=0) / l.sum()
        f = np.exp(m - m.max())
        return (f @ o) / (f @ l)


# ------------------------------------------------------------------ the probes
def code_matrix():
    return np.random.default_rng(CODE_SEED).choice(np.array([-1.0, 1.0], np.float32), size=(ATT_MAXK, 64))


def code_max_offdiag(code):
    g = code.astype(np.float64) @ code.astype(np.float64).T
    np.fill_diagonal(g, -64)
    return float(g.max())


def probe_values(pair, T, positive=False):
    """v [T][64] = non-zero integers / 16 (bf16-exact, |v| < 8) that differ from key to key in every column and from pair to pair"""
    j, e = np.arange(T)[:, None], np.arange(64)[None, :]
    mag = (j * 37 + e * 11 + pair * 53) % 127 + 1
    sign = 1 if positive else np.where((j + e) % 2 == 0, 1, -1)
    return (mag * sign / 16.0).astype(np.float32)


def nan_outside(a, lo, hi):
    """a [T][64] with every row outside [lo, hi] set to NaN"""
    a = np.array(a, np.float32)
    a[:lo] = np.nan
    a[hi + 1:] = np.nan
    return a


def counting_marks(n_pairs, n, NS, priority=None):
    """marks [n_pairs][64] of relative key positions (-1: column unused): the keys in `priority` order (default: the boundary keys,
    then every other key in a fixed shuffled order) dealt round-robin to the pairs, at most 64 a pair, each key marked once."""
    if priority is None:
        first = boundary_keys(n, NS)
        rest = [int(x) for x in np.random.default_rng(n).permutation(n) if int(x) not in first]
        priority = first + rest
    marks = np.full((n_pairs, 64), -1, np.int64)
    for i, key in enumerate(priority[:n_pairs * 64]):
        marks[i % n_pairs, (i // n_pairs + 5 * (i % n_pairs)) % 64] = key
    return marks


def counting_probe(n_pairs, T, lo, hi, NS, seed=0, priority=None):
    """-> q [n_pairs][64] (random: a key row that is not 0 would move the weights), k, v [n_pairs][T][64], marks [n_pairs][64].
    lo / hi: the pairs' key ranges (scalars or [n_pairs]); they must have one length n.  Pair p's keys are 0 inside its range."""
    lo, hi = np.broadcast_to(lo, (n_pairs,)), np.broadcast_to(hi, (n_pairs,))
    n = int(hi[0] - lo[0] + 1)
    assert np.all(hi - lo + 1 == n)
    marks = counting_marks(n_pairs, n, NS, priority)
    q = np.random.default_rng(seed).standard_normal((n_pairs, 64)).astype(np.float32)
    k = np.full((n_pairs, T, 64), np.nan, np.float32)
    v = np.full((n_pairs, T, 64), np.nan, np.float32)
    for p in range(n_pairs):
        k[p, lo[p]:hi[p] + 1] = 0.0
        v[p, lo[p]:hi[p] + 1] = 0.0
        for e in range(64):
            if marks[p, e] >= 0:
                v[p, lo[p] + marks[p, e], e] = 1.0
    return q, k, v, marks


def counting_check(out, marks, n):
    """out [n_pairs][64] (f32 or f64) against the counting answer: 1 / n to one bf16 ulp where a key is marked, exactly 0 elsewhere.
    Returns the list of (pair, column, got) that miss -- empty when the probe accepts."""
    bad = []
    want, ulp = 1.0 / n, bf16_ulp(1.0 / n)
    for p in range(marks.shape[0]):
        for e in range(64):
            got = float(out[p, e])
            ok = abs(got - want) <= ulp if marks[p, e] >= 0 else got == 0.0
            if not ok:       # (NaN fails both)
                bad.append((p, e, got))
    return bad


def selection_probe(code, sel, T, lo, hi):
    """one pair per entry of sel (relative key positions, sel[p] <= hi[p] - lo[p]): q [P][64], k, v [P][T][64], want [P][64] = the
    selected V rows.  The code rows are those of the RELATIVE positions, so a pair's scores do not depend on its offset."""
    P = len(sel)
    lo, hi = np.broadcast_to(lo, (P,)), np.broadcast_to(hi, (P,))
    q = np.zeros((P, 64), np.float32)
    k = np.full((P, T, 64), np.nan, np.float32)
    v = np.full((P, T, 64), np.nan, np.float32)
    want = np.zeros((P, 64), np.float32)
    for p in range(P):
        n = int(hi[p] - lo[p] + 1)
        assert 0 <= sel[p] < n
        k[p, lo[p]:hi[p] + 1] = 16.0 * code[:n]
        v[p, lo[p]:hi[p] + 1] = probe_values(p, n)
        q[p] = code[sel[p]]
        want[p] = v[p, lo[p] + sel[p]]
    return q, k, v, want


def two_peak_lead(code, a, b, n):
    """score(a) = score(b) minus the largest other score among the first n keys (scores as the kernel scales them: q . k / 8)"""
    s = 2.0 * (code[:n].astype(np.float64) @ (code[a] + code[b]).astype(np.float64))
    assert s[a] == s[b]
    rest = np.delete(s, [a, b])
    return float(s[a] - rest.max()) if rest.size else float("inf")


def two_peak_probe(code, peaks, T, n):
    """one pair per (a, b) of peaks over keys [0, n): q = code[a] + code[b], want = (v[a] + v[b]) / 2 (bf16-exact: positive
    integers / 16 whose sum is below 256).  Asserts the lead over the third score."""
    P = len(peaks)
    q = np.zeros((P, 64), np.float32)
    k = np.full((P, T, 64), np.nan, np.float32)
    v = np.full((P, T, 64), np.nan, np.float32)
    want = np.zeros((P, 64), np.float32)
    for p, (a, b) in enumerate(peaks):
        assert a != b and 0 <= a < n and 0 <= b < n
        assert two_peak_lead(code, a, b, n) >= MIN_LEAD, (a, b, two_peak_lead(code, a, b, n))
        k[p, :n] = 16.0 * code[:n]
        v[p, :n] = probe_values(p, n, positive=True)
        q[p] = code[a] + code[b]
        want[p] = (v[p, a] + v[p, b]) / 2
        assert np.array_equal(bf16(want[p]), want[p])
    return q, k, v, want


def two_peak_pairs(code, n, NS):
    """(a, b) with: same stream and different blocks in both orders, different streams and the same block, different streams and
    blocks, the first and the last key -- each moved forward to the nearest choice whose lead is >= MIN_LEAD"""
    g = code[:n].astype(np.float64) @ code[:n].astype(np.float64).T

    def lead(a, b):
        s = 2.0 * (g[a] + g[b])
        top = s[a]
        s[[a, b]] = -np.inf
        return top - s.max() if n > 2 else np.inf

    def first(pairs):
        """the first candidate whose lead is at least 64, else the best one; None when no candidate reaches MIN_LEAD"""
        best = None
        for a, b in pairs:
            l = lead(a, b)
            if best is None or l > best[0]:
                best = (l, a, b)
            if l >= 64:
                break
        return None if best is None or best[0] < MIN_LEAD else (best[1], best[2])

    i = np.arange(n)
    b0, b1 = i[block_of(i, NS) == 0], i[block_of(i, NS) == 1]
    same = [(int(a), int(b)) for a in b0[:64] for b in b1 if stream_of(a, NS) == stream_of(b, NS)][:400]
    cats = [same, [(b, a) for a, b in same],
            [(int(a), int(b)) for a in b0[:24] for b in b0 if stream_of(a, NS) != stream_of(b, NS) and a < b][:400],
            [(int(a), int(b)) for a in b0[8:32] for b in b1 if stream_of(a, NS) != stream_of(b, NS)][:400]]
    out = [p for p in map(first, cats) if p is not None]
    if n >= 2 and lead(0, n - 1) >= MIN_LEAD:
        out.append((0, n - 1))
    return out


def spread_case(n_pairs, T, lo, hi, seed):
    """q [P][64] with |q| ~ 24 (scores q . k / 8 of standard deviation ~3: tens of keys matter), k ~ N(0, 1) rounded to bf16, v of
    mixed sign and a per-element magnitude 2^-3 .. 2^3 -- no common ramp; NaN outside [lo, hi]."""
    rng = np.random.default_rng(seed)
    lo, hi = np.broadcast_to(lo, (n_pairs,)), np.broadcast_to(hi, (n_pairs,))
    q = (3.0 * rng.standard_normal((n_pairs, 64))).astype(np.float32)
    k = bf16(rng.standard_normal((n_pairs, T, 64)))
    v = bf16(rng.standard_normal((n_pairs, T, 64)) * 2.0 ** rng.integers(-3, 4, (n_pairs, T, 64)))
    for p in range(n_pairs):
        k[p], v[p] = nan_outside(k[p], lo[p], hi[p]), nan_outside(v[p], lo[p], hi[p])
    return q, k, v


def spread_gate(ref, vmax, extra=0.0):
    """the per-element bound |out - ref| <= 2^-8 |ref| + 2^-12 max|v| (+ extra): the half-ulp of the bf16 output, and headroom for
    the f32 arithmetic -- at most 24 sequential FMAs per lane chain, 6 shuffle adds, 8 merges and __expf at |x| <= 40 stay
    below 2^-17 max|v|, so 2^-12 leaves 32x"""
    return 2.0 ** -8 * np.abs(ref) + 2.0 ** -12 * vmax + extra


def spread_ratio(out, ref, vmax, extra=0.0):
    """worst |out - ref| / gate over the elements (NaN counts as inf)"""
    r = np.abs(np.asarray(out, np.float64) - ref) / spread_gate(ref, vmax, extra)
    return float(np.where(np.isnan(r), np.inf, r).max())


def heads(a, rows, H):
    """pair-major [rows * H][...] -> what the hooks take: q [rows][H * 64] or k / v [rows][H][T][64]"""
    a = np.asarray(a)
    if a.ndim == 2:
        return np.ascontiguousarray(a.reshape(rows, H * 64))
    return np.ascontiguousarray(a.reshape(rows, H, a.shape[1], 64))
