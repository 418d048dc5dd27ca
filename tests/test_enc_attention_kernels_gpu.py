"""enc_attn_kernel (csrc/enc_kernels.hip) at kernel level, through wmdbg_enc_attention / wmdbg_enc_attention_ex with both row-sum
variants (debug knob enc_attn_mfma_sum 0 and 1).  References, bounds and probe builders: tests/enc_attn_ref.py, held to their
conditions on the CPU by test_enc_attn_ref_cpu.py.

Spread           every element within the derived bound u (A + |ref|) + f32 terms (SUM_MFMA: u (A + 2 |ref|) + f32 terms), at every
                 S at which the ring's prologue, the tile loop or the masked last tile differ, one and six pairs, and nine live
                 pairs of a grid padded to sixteen; on N(0, 1) inputs and on "peaked" ones (q x 2.5), whose rows take hundreds of
                 late moves of the softmax reference with old mass that still matters.
Threshold        one-hot queries against integer keys: every weight is a dyadic rational, gated at half a bf16 ulp (+ the f32
                 terms that remain) on both sides of the 2^8 threshold, with the moving key in tile 1, a middle and the last
                 tile, with the 32 queries of a wave disagreeing, and with two equal maxima in different tiles.
Chunks, heads    selection (a different permutation per pair) and counting at (B, H, S) = (3, 2, 1500) and (2, 5, 129); a chunk
                 of three gives the bits of the chunk alone.
Masked keys      NaN in the 64 rows the last K tile reads behind the keys changes no bit."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_attn_ref as E   # noqa: E402

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
_REF = {}
_WORST = {}


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_enc_attention.argtypes = [vp, vp, vp, vp, ip, ip, ip, vp]
    c.lib.wmdbg_enc_attention_ex.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, vp]
    c.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ip]
    c.lib.wm_last_error.restype = ctypes.c_char_p
    yield c
    c.lib.wmdbg_set_tuning(b"reset", 0)
    c.close()
    for k in sorted(_WORST):               # (shown with -s) largest |got - ref| / bound
        print("error / bound, %-28s %.4f" % (k, _WORST[k]))


@contextlib.contextmanager
def row_sum(dbg, mfma_sum):
    try:
        assert dbg.lib.wmdbg_set_tuning(b"enc_attn_mfma_sum", mfma_sum) == 0
        yield
    finally:
        dbg.lib.wmdbg_set_tuning(b"reset", 0)


def P(a):
    return a.ctypes.data_as(vp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def attention(dbg, q, k, v, H, flags=0):
    """one launch; the output starts as NaN, so an element the kernel never wrote shows"""
    B, S, d = q.shape
    assert d == H * 64
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    out = np.full((B, S, d), np.nan, np.float32)
    if flags:
        st = dbg.lib.wmdbg_enc_attention_ex(dbg.handle, P(q), P(k), P(v), B, H, S, flags, P(out))
    else:
        st = dbg.lib.wmdbg_enc_attention(dbg.handle, P(q), P(k), P(v), B, H, S, P(out))
    assert st == 0, dbg.lib.wm_last_error()
    return out


def spread(case):
    if case not in _REF:
        B, H, S, kind = case
        q, k, v = E.spread_inputs(B, H, S, kind)
        _REF[case] = (q, k, v, E.restate(q, k, v, H))
    return _REF[case]


def case_id(c):
    return "B%d-H%d-S%d-%s" % c


# ------------------------------------------------------------------ spread: every element at the bound
@pytest.mark.parametrize("mfma_sum", [0, 1])
@pytest.mark.parametrize("case", E.spread_cases(), ids=case_id)
def test_every_element_within_the_derived_bound(dbg, case, mfma_sum):
    B, H, S, kind = case
    q, k, v, r = spread(case)
    with row_sum(dbg, mfma_sum):
        out = attention(dbg, q, k, v, H)
    assert np.isfinite(out).all(), "an element is not finite (never written?)"
    ratio = np.abs(out.astype(np.float64) - r.ref) / r.bound[mfma_sum]
    worst = float(ratio.max())
    print("%s mfma_sum %d: error / bound = %.4f" % (case_id(case), mfma_sum, worst))
    key = "%s S %s sum %d" % (kind, "1500" if S == 1500 else "< 200", mfma_sum)
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    assert worst <= 1.0, (worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


# ------------------------------------------------------------------ threshold probes with exact answers
PROBES = E.threshold_cases()


@pytest.mark.parametrize("name,amp,kint", PROBES, ids=[p[0] for p in PROBES])
def test_threshold_probe(dbg, name, amp, kint):
    B, H, S = amp.shape
    q, k, v, exact, _ = E.threshold_probe(amp, kint)
    # the hook's rounding, recomputed here: the pre-scaled query is one-hot and holds exactly amp
    qs = E.prescale(q)
    for h in range(H):
        e0 = h * 64 + E.probe_dim(h)
        assert np.array_equal(qs[:, :, e0].astype(np.float64), amp[:, h])
    assert not np.delete(qs, [g * 64 + E.probe_dim(g) for g in range(H)], axis=2).any()
    gate = E.probe_gate(exact, S)
    for mfma_sum in (0, 1):
        with row_sum(dbg, mfma_sum):
            out = attention(dbg, q, k, v, H)
        err = np.abs(out.astype(np.float64) - exact)
        bad = np.argwhere(~(err <= gate))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.where(gate > 0, err / gate, 0.0).max())
        print("%s mfma_sum %d: error / gate = %.4f" % (name, mfma_sum, worst))
        _WORST["probe " + name.split("-")[0]] = max(_WORST.get("probe " + name.split("-")[0], 0.0), worst)
        assert bad.size == 0, (name, mfma_sum, len(bad), bad[:6], out[tuple(bad[:6].T)], exact[tuple(bad[:6].T)])


# ------------------------------------------------------------------ chunks and heads
@pytest.mark.parametrize("mfma_sum", [0, 1])
@pytest.mark.parametrize("B,H,S", [(3, 2, 1500), (2, 5, 129)])
def test_selection_and_counting_per_pair(dbg, B, H, S, mfma_sum):
    """Selection: query i of pair (b, h) selects key pi_bh(i), another permutation for every pair, so the output row is
    v[b][pi_bh(i)][h] bit for bit: b * H + h is told from h * B + b.  Counting: q = 0, every key weighs 1 / S, and pair (b, h)'s
    64 columns mark another 64 keys."""
    q, k, v, want = E.selection_probe(B, H, S)
    zero = np.zeros((B, H, S))
    qc, kc, vc, exact, marks = E.threshold_probe(zero, zero.astype(np.int64))
    assert len({tuple(m) for m in marks.reshape(-1, 64)}) == B * H
    with row_sum(dbg, mfma_sum):
        out = attention(dbg, q, k, v, H)
        cnt = attention(dbg, qc, kc, vc, H)
    miss = np.argwhere((bits(out) != bits(want)).any(axis=2))
    assert miss.size == 0, ("selection: (chunk, query) rows whose output is not v[pi(i)]", len(miss), miss[:10])
    assert np.array_equal(np.unique(exact), np.array([1.0 / S]))
    bad = np.argwhere(~(np.abs(cnt.astype(np.float64) - exact) <= E.probe_gate(exact, S)))
    assert bad.size == 0, ("counting: (chunk, query, column) not counted once", len(bad), bad[:8], cnt[tuple(bad[:8].T)], 1.0 / S)


@pytest.mark.parametrize("mfma_sum", [0, 1])
@pytest.mark.parametrize("S,kind", [(1500, "peaked"), (129, "normal"), (28, "peaked")])
def test_chunk_of_three_is_bit_identical_to_the_chunk_alone(dbg, S, kind, mfma_sum):
    """Chunk b's last K tile runs past its S rows into chunk b + 1's (the last chunk's into the 64 rows behind); the mask makes
    that invisible, so a chunk does not depend on its neighbours."""
    q, k, v, _ = spread((3, 2, S, kind))
    with row_sum(dbg, mfma_sum):
        all3 = attention(dbg, q, k, v, 2)
        for b in range(3):
            alone = attention(dbg, q[b:b + 1], k[b:b + 1], v[b:b + 1], 2)
            assert np.array_equal(bits(all3[b]), bits(alone[0])), (S, b)


# ------------------------------------------------------------------ masked keys
@pytest.mark.parametrize("mfma_sum", [0, 1])
@pytest.mark.parametrize("S", [1500, 129, 28])
def test_nan_behind_the_keys_changes_no_bit(dbg, S, mfma_sum):
    """The kernel masks the SCORE of a key >= S after the product, so whatever the K tile holds there -- NaN here, in all 64 rows
    behind the chunk -- must not reach the output.  (The V^T pad columns are zero by contract: wmdbg_encode_layer_qkv guards
    that side.)"""
    q, k, v = E.spread_inputs(1, 2, S, "normal")
    with row_sum(dbg, mfma_sum):
        clean = attention(dbg, q, k, v, 2)
        dirty = attention(dbg, q, k, v, 2, flags=1)
    assert np.isfinite(dirty).all()
    assert np.array_equal(bits(clean), bits(dirty))


def test_hook_rejects_unknown_flags(dbg):
    q = np.zeros((1, 4, 64), np.float32)
    out = np.zeros_like(q)
    assert dbg.lib.wmdbg_enc_attention_ex(dbg.handle, P(q), P(q), P(q), 1, 1, 4, 2, P(out)) == 1
