"""CPU checks of tests/dec_attn_ref.py: the conditions the exact-answer probes of tests/test_dec_attention_kernels_gpu.py rest on,
and the evidence that they bite -- each known-wrong variant of the streamed restatement (dec_attn_ref.FAULTS) is rejected by
the probes meant for it -- while the value gate the suite had before (test_kernels_gpu.py::test_decode_attention) lets a
dropped and a doubled key through on its own inputs.

MEASURED (numpy, f64; the old gate is max|out - ref| <= 2^-8 max(1, max|ref|) on q, k ~ N(0, 1), v ~ N(0, 1) + ramp, seed
T + n_keys, the faulted output rounded to bf16 like the kernel's):
  shape (B, H, T, n_keys)   gate      last key dropped      one key counted twice
  (1, 1, 1500, 1500)        0.0039    err 0.0022: ACCEPTED  accepted for 1309 of the 1500 keys
  (2, 2, 1500, 1500)        0.0042    err 0.0045: rejected  accepted for 709 of the 1500 keys
  (3, 2, 1500, 1500)        0.0042    err 0.0068: rejected  accepted for 582 of the 1500 keys
(the more pairs a case has, the likelier one of them gives the dropped key a large weight; without the bf16 rounding of the
output the (2, 2) case accepts the dropped key too, at 0.0032.)
So at the cross-attention's real key count the old gate misses a doubled key at 40 to 90 % of the positions and a dropped last key in its one-pair case;
every equal-bits test of the suite passes then too, because all launch forms share the block arithmetic.
ON THE MI355X, a build whose attn_block masks the last key of a partial block (an experiment, not committed): the old gate
fails 13 of its 17 cases and passes the one-pair case (1, 1, 1500, 1500) as computed above (the others that pass have one key
or a full block); all 64 equal-bits tests of the candidate, teacher-panel and prompt-panel kernels pass, as they must -- the
wrong arithmetic is shared; test_dec_attention_kernels_gpu.py fails in 10 of its 16 test functions (those that pass use
full blocks, compare bits between launches, or launch nothing).
  * the counting probe rejects both (the marked column reads 0 or 2 / n instead of 1 / n);
  * the selection probe's answer is exact: its f64 softmax differs from v[j*] by at most 1536 * 16 * exp(-56) = 1.2e-20
    in the worst case the margin allows and by 0 (< 3e-24) on the seed's actual scores.
"""
import numpy as np
import pytest

import dec_attn_ref as A

CODE = A.code_matrix()


def test_row_geometry_and_boundary_keys():
    assert A.boundary_keys(1500, 8) == [0, 1, 7, 8, 63, 64, 65, 255, 256, 257, 511, 512, 1279, 1280, 1498, 1499]
    assert A.boundary_keys(448, 4) == [0, 1, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 446, 447]
    assert A.boundary_keys(1, 8) == [0] and A.boundary_keys(9, 4) == [0, 1, 7, 8]
    for NS in (4, 8):
        i = np.arange(A.ATT_MAXK)
        # (stream, row group, load, block) names every row once
        key = ((A.block_of(i, NS) * A.U + A.load_of(i, NS)) * NS + A.stream_of(i, NS)) * 8 + i % 8
        assert np.array_equal(key, i)
        assert A.block_of(NS * 32 - 1, NS) == 0 and A.block_of(NS * 32, NS) == 1
    assert A.ATT_MAXK // (8 * 8 * A.U) == 6          # six full blocks: the deep kernel's up-front loads


def test_bf16_rounding_is_the_hooks():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e-5, 255.0, 1 / 3, np.inf], np.float32)
    want = np.array([1.0, 1.0, 1.015625, -3.0040e-5, 255.0, 0.333984375, np.inf], np.float32)
    got = A.bf16(x)
    assert np.array_equal(got[[0, 1, 2, 4, 5, 6]], want[[0, 1, 2, 4, 5, 6]])       # ties to even, both ways
    assert got.view(np.uint32)[3] & 0xffff == 0 and np.isnan(A.bf16(np.float32(np.nan)))
    assert A.bf16_ulp(1.0) == 2.0 ** -7 and A.bf16_ulp(1 / 1500) == 2.0 ** -18


def test_the_code_matrix_keeps_its_margin():
    """Nobody changes the seed into a weak probe: the largest off-diagonal code . code is at most 40 of 64 (36 with the seed), so
    a selected score (128) leads every other (<= 80) by at least 48 -- and by MIN_LEAD = 56 with the seed's 36."""
    m = A.code_max_offdiag(CODE)
    assert m <= 40
    assert 2 * (64 - m) >= A.MIN_LEAD
    assert set(np.unique(CODE)) == {-1.0, 1.0} and CODE.shape == (1536, 64)
    v = A.probe_values(3, 1536)
    assert np.array_equal(A.bf16(v), v) and np.all(v != 0) and np.abs(v).max() < 8
    assert np.all(np.abs(np.diff(v, axis=0)) > 0)          # neighbouring keys differ in every column


def test_selection_answer_is_exact_for_every_key_count():
    worst = 0.0
    for n in range(1, 1537):
        sel = (n * 7) // 11 % n if n % 5 else n - 1
        q, k, v, want = A.selection_probe(CODE, [sel], n, 0, n - 1)
        o = A.attention_f64(q[0], k[0], v[0], 0, n - 1)
        worst = max(worst, float(np.abs(o - want[0]).max()))
    print("selection probe: largest |f64 answer - v[j*]| over n_keys 1 .. 1536 = %.3g" % worst)
    assert worst < 3e-24
    # ... and at an offset (the ragged self-attention): NaN in front of and behind the range is never touched
    q, k, v, want = A.selection_probe(CODE, [5, 40], 448, [100, 7], [140, 47])
    assert np.isnan(k[0, 99]).all() and np.isnan(v[0, 141]).all()
    for p, (lo, hi) in enumerate(((100, 140), (7, 47))):
        assert np.array_equal(A.attention_f64(q[p], k[p], v[p], lo, hi), want[p].astype(np.float64))


@pytest.mark.parametrize("NS,n", [(8, 1500), (8, 1536), (8, 300), (8, 9), (4, 448), (4, 130), (4, 2)])
def test_two_peak_answer_is_exact(NS, n):
    pk = A.two_peak_pairs(CODE, n, NS)
    assert pk
    if n in (1500, 1536, 130, 2):        # counts the GPU tests use: the first and the last key are a pair (at 448 their lead is too small)
        assert pk[-1] == (0, n - 1)
    if n >= 2 * NS * 32:
        (a, b), (c, d) = pk[0], pk[1]
        assert A.stream_of(a, NS) == A.stream_of(b, NS) and A.block_of(a, NS) < A.block_of(b, NS) and (c, d) == (b, a)
        assert any(A.stream_of(a, NS) != A.stream_of(b, NS) and A.block_of(a, NS) == A.block_of(b, NS) for a, b in pk)
        assert any(A.stream_of(a, NS) != A.stream_of(b, NS) and A.block_of(a, NS) != A.block_of(b, NS) for a, b in pk)
    q, k, v, want = A.two_peak_probe(CODE, pk, n, n)
    for p, (a, b) in enumerate(pk):
        assert A.two_peak_lead(CODE, a, b, n) >= A.MIN_LEAD
        assert np.abs(A.attention_f64(q[p], k[p], v[p], 0, n - 1) - want[p]).max() < 1e-20
        assert np.all(want[p] != 0)


def test_counting_marks_cover_every_key_once():
    for n_pairs, n, NS in ((24, 1536, 8), (6, 1500, 8), (4, 448, 4), (7, 448, 4), (6, 5, 8)):
        m = A.counting_marks(n_pairs, n, NS)
        used = m[m >= 0]
        assert len(used) == len(set(used.tolist())) == min(n, n_pairs * 64)
        if n <= n_pairs * 64:
            assert set(used.tolist()) == set(range(n))           # 24 pairs cover all 1536 keys, 7 pairs all 448
        assert set(A.boundary_keys(n, NS)) <= set(used.tolist())
    q, k, v, marks = A.counting_probe(24, 1536, 0, 1535, 8)
    out = np.stack([A.attention_f64(q[p], k[p], v[p], 0, 1535) for p in range(24)])
    assert A.counting_check(out, marks, 1536) == []
    assert A.counting_check(A.bf16(out), marks, 1536) == []


# ------------------------------------------------------------------ the probes bite
def run_probe(kind, NS, n, fault, fault_key, T=None):
    """-> True when the probe ACCEPTS the (faulted) streamed restatement"""
    T = T or n + 1                      # one NaN row behind the last key
    st = lambda q, k, v: A.streamed_attention(q, k, v, 0, n - 1, NS, fault, fault_key)
    if kind == "counting":
        q, k, v, marks = A.counting_probe(6, T, 0, n - 1, NS, priority=[fault_key] + [j for j in range(n) if j != fault_key])
        out = np.stack([st(q[p], k[p], v[p]) for p in range(6)])
        return A.counting_check(A.bf16(out), marks, n) == []
    if kind == "selection":
        q, k, v, want = A.selection_probe(CODE, [fault_key], T, 0, n - 1)
        return np.array_equal(A.bf16(st(q[0], k[0], v[0])), want[0])
    if kind == "two_peak":
        pk = [p for p in A.two_peak_pairs(CODE, n, NS)]
        q, k, v, want = A.two_peak_probe(CODE, pk, T, n)
        return all(np.array_equal(A.bf16(st(q[p], k[p], v[p])), want[p]) for p in range(len(pk)))
    q, k, v = A.spread_case(4, T, 0, n - 1, 11)
    vmax = float(np.nanmax(np.abs(v)))
    return all(A.spread_ratio(A.bf16(st(q[p], k[p], v[p])), A.attention_f64(q[p], k[p], v[p], 0, n - 1), vmax) <= 1.0 for p in range(4))


# (fault, the key it acts on, the probes that must reject it); n = 437 is a partial second block of the cross-attention, its
# last key 436; key 300 sits in block 1, behind a block whose maximum is lower: the rescale and the merge matter there
BITES = [("drop_last_of_partial_block", 436, ("counting", "selection")),
         ("count_twice", 300, ("counting",)),
         ("count_twice", 0, ("counting", "two_peak")),
         ("no_rescale", 300, ("selection", "two_peak", "spread")),
         ("merge_unaligned", 300, ("selection", "two_peak", "spread")),
         ("swap_v_rows", 300, ("selection",)),
         ("swap_v_rows", 0, ("two_peak",)),
         ("read_past_end", 436, ("counting", "selection", "two_peak", "spread"))]


@pytest.mark.parametrize("NS", [8, 4])
def test_every_probe_accepts_the_streamed_restatement(NS):
    n = 437
    q, k, v = A.spread_case(2, n, 0, n - 1, 3)
    for p in range(2):
        assert np.abs(A.streamed_attention(q[p], k[p], v[p], 0, n - 1, NS) - A.attention_f64(q[p], k[p], v[p], 0, n - 1)).max() < 1e-12
    for kind in ("counting", "selection", "two_peak", "spread"):
        assert run_probe(kind, NS, n, None, 300), kind


@pytest.mark.parametrize("fault,key,kinds", BITES)
@pytest.mark.parametrize("NS", [8, 4])
def test_known_wrong_kernels_are_rejected(NS, fault, key, kinds):
    for kind in kinds:
        assert not run_probe(kind, NS, 437, fault, key), (fault, kind)


def test_what_the_counting_probe_cannot_see_the_others_do():
    """Stated so that nobody reads more into a probe than it holds: with uniform weights no maximum ever moves and a V row swap
    keeps the sum, so the counting probe ACCEPTS no_rescale and swap_v_rows; a doubled key that is the selected one leaves the
    selection answer unchanged.  Each is rejected by another probe (BITES)."""
    assert run_probe("counting", 8, 437, "no_rescale", 300)
    assert run_probe("counting", 8, 437, "swap_v_rows", 300)     # (a marked row swapped with its neighbour moves no sum)
    assert run_probe("selection", 8, 437, "count_twice", 300)


# ------------------------------------------------------------------ the spread case
@pytest.mark.parametrize("NS,T,n", [(8, 1500, 1500), (4, 448, 448), (8, 1500, 437), (4, 448, 37)])
def test_f32_restatement_with_another_summation_order_passes_the_spread_gate(NS, T, n):
    q, k, v = A.spread_case(6, T, 0, n - 1, 7)
    vmax = float(np.nanmax(np.abs(v)))
    worst, eff = 0.0, []
    for p in range(6):
        ref = A.attention_f64(q[p], k[p], v[p], 0, n - 1)
        worst = max(worst, A.spread_ratio(A.attention_f32_plain(q[p], k[p], v[p], 0, n - 1), ref, vmax))
        s = k[p, :n].astype(np.float64) @ q[p] / 8
        w = np.exp(s - s.max())
        eff.append(float(w.sum() ** 2 / (w ** 2).sum()))
        assert 1.5 <= s.std() <= 4.5
    print("spread case NS %d n %d: f32 restatement at %.3f of the gate; keys that matter (1 / sum w^2): %s" % (NS, n, worst, np.round(eff, 1)))
    assert worst <= 1.0
    assert (v[:, :n] > 0).any() and (v[:, :n] < 0).any()
    assert n < 400 or np.abs(np.nanmean(v[:, :n], axis=(0, 1))).max() < 0.5   # no common ramp


# ------------------------------------------------------------------ the evidence: the old gate
def old_gate_case(B, H, T, n):
    """test_decode_attention's inputs, its reference and its bound"""
    rng = np.random.default_rng(T + n)
    q = rng.standard_normal((B, H * 64)).astype(np.float32)
    k = A.bf16(rng.standard_normal((B, H, T, 64)))
    v = A.bf16(rng.standard_normal((B, H, T, 64)) + np.linspace(-1, 1, 64))
    s = np.einsum("bhe,bhte->bht", q.reshape(B, H, 64).astype(np.float64), k[:, :, :n].astype(np.float64)) / 8
    p = np.exp(s - s.max(-1, keepdims=True))
    vv = v[:, :, :n].astype(np.float64)
    out = lambda w: np.einsum("bht,bhte->bhe", w, vv) / w.sum(-1)[..., None]
    ref = out(p)
    return p, out, ref, 2.0 ** -8 * max(1.0, np.abs(ref).max())


def test_the_old_value_gate_accepts_a_dropped_and_a_doubled_key():
    for shape, must_accept_drop in (((1, 1, 1500, 1500), True), ((2, 2, 1500, 1500), False), ((3, 2, 1500, 1500), False)):
        p, out, ref, gate = old_gate_case(*shape)
        w = p.copy()
        w[..., -1] = 0                                    # the last key of the partial sixth block is dropped
        e_drop = float(np.abs(A.bf16(out(w)) - ref).max())
        acc = 0
        for j in range(0, 1500, 1):
            w = p.copy()
            w[..., j] *= 2                                # key j is counted twice
            acc += float(np.abs(A.bf16(out(w)) - ref).max()) <= gate
        print("old gate %s: bound %.3g; last key dropped: err %.3g; a doubled key accepted for %d of 1500 keys" % (shape, gate, e_drop, acc))
        assert (e_drop <= gate) or not must_accept_drop
        assert acc >= 500
