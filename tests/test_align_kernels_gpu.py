"""GPU unit tests of the alignment kernels of wm_align (csrc/align.hip) through the wmdbg_align_* hooks: the column
statistics and cost-matrix kernels (wmdbg_align_matrix) against an fp64 restatement of find_alignment steps 2-5 on the same
f32 queries and bf16-rounded keys, and the token-probability kernel (wmdbg_align_token_prob) against an fp64 softmax.
The median is 1-Lipschitz in the max norm, so max|x - x_ref| bounds the kernels' error directly.  tests/test_align_cpu.py
reuses CASES, inputs() and GATES to show that known-wrong variants of the algorithm move x far past these gates."""
import json
import os

import numpy as np
import pytest
import torch

from test_align_cpu import alignment_matrix

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD     # the bits wmdbg_align_matrix pre-fills x with
MEASURED = {}

# max|x - x_ref| per input regime, gates >= 3x the largest value measured on an MI355X over every case of the regime: normal
# 4.4e-6, peaked 1.8e-5, cv1e-2 7.6e-5, cv1e-3 1.3e-3 (the one-pass variance before: 2.9e-2, and 0.27 or inf / nan) (with
# $WM_MEASURED_DIR set, the tests write what they measure to align_kernels_measured.json there)
GATES = {"normal": 2e-5, "peaked": 6e-5, "cv1e-2": 3e-4, "cv1e-3": 5e-3}
# q and k ~ N(0, scale^2): the per-frame coefficient of variation of the probabilities over the rows is ~ scale^2
SCALE = {"normal": 1.0, "peaked": 1.0, "cv1e-2": 0.1, "cv1e-3": 0.03}
# decoder layers, heads per layer, alignment heads (the order the mean adds them)
HEADS = {"one": (2, 3, [(1, 2)]),
         "three": (4, 6, [(0, 5), (2, 1), (3, 3)]),
         "large-v2": (32, 20, [(l, h) for l in range(16, 32) for h in range(20)])}
# (regime, heads, S, medfilt_width, qk_scale, chunks [(n_text, n_frames)]); M = n_frames // 2, T = S + n + 2 <= 448.
# Widths 1-7 take the register median, 9-31 the LDS one; M runs over 1, 2, h, h + 1 and the 16-row / 64-frame tile edges.
CASES = [
    ("normal", "one", 1, 1, 1.0, [(1, 2), (14, 4), (15, 31), (16, 32), (17, 35), (64, 3000)]),
    ("normal", "three", 3, 3, 0.37, [(16, 2), (63, 5), (1, 126), (14, 129), (17, 130), (443, 3000)]),
    ("normal", "three", 4, 31, 2.5, [(1, 30), (15, 33), (64, 34), (16, 254), (17, 258), (442, 2998)]),
    ("normal", "large-v2", 3, 7, 1.0, [(40, 3000)]),
    ("peaked", "three", 3, 5, 1.0, [(1, 4), (17, 6), (63, 1234), (64, 2999), (443, 3000)]),
    ("peaked", "one", 1, 9, 2.5, [(14, 8), (15, 10), (16, 128), (445, 1500)]),
    ("peaked", "three", 4, 1, 1.0, [(1, 3), (63, 127), (442, 3000)]),
    ("cv1e-2", "three", 3, 7, 1.0, [(1, 6), (16, 8), (63, 1234), (443, 3000)]),
    ("cv1e-2", "one", 4, 15, 2.5, [(14, 14), (17, 16), (64, 3000), (442, 1500)]),
    ("cv1e-2", "three", 1, 1, 0.37, [(1, 2), (15, 129), (445, 2999)]),
    ("cv1e-3", "three", 1, 9, 1.0, [(1, 8), (15, 10), (64, 1234), (445, 3000)]),
    ("cv1e-3", "one", 3, 31, 0.37, [(16, 30), (17, 32), (63, 2999), (443, 3000)]),
    ("cv1e-3", "three", 4, 3, 2.5, [(1, 2), (14, 4), (63, 130), (442, 3000)]),
]


def case_id(c):
    return "%s-%s-S%d-w%d-qk%g" % c[:5]


def inputs(case, seed):
    """(q f32 [B][Tq][J][64], keys f32 [L][B][H][1500][64]).  q rows past each chunk's T and the keys of every (layer, head)
    that is no alignment head are NaN: the kernels must never read them.  "peaked": every row of a head has one dominant key
    frame, q = (2 k[f] + noise) / qk_scale: after qk_scale a lead of ~16 (natural-log units) over the other frames."""
    regime, hk, S, _, qk_scale, chunks = case
    L, H, heads = HEADS[hk]
    B, J, sd = len(chunks), len(heads), SCALE[regime]
    Tq = S + max(n for n, _ in chunks) + 2
    rng = np.random.default_rng(seed)
    keys = np.full((L, B, H, 1500, 64), np.nan, dtype=np.float32)
    q = np.full((B, Tq, J, 64), np.nan, dtype=np.float32)
    for b, (n, nf) in enumerate(chunks):
        T, M = S + n + 2, nf // 2
        for j, (l, h) in enumerate(heads):
            keys[l, b, h] = rng.standard_normal((1500, 64)) * sd
            if regime == "peaked":
                f = rng.integers(0, M, size=T)
                q[b, :T, j] = (2.0 * keys[l, b, h, f] + 0.3 * rng.standard_normal((T, 64))) / qk_scale
            else:
                q[b, :T, j] = rng.standard_normal((T, 64)) * sd
    return q, keys


def bf16(x):
    """round to the nearest bf16, ties to even (the rounding the hook applies to the keys)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def head_scores(q, keys, heads, b, T, M):
    """q.k / 8 in f64 of chunk b, every head: [J][T][M] (the keys rounded to bf16 as the cache holds them)"""
    out = []
    for j, (l, h) in enumerate(heads):
        k = torch.as_tensor(bf16(keys[l, b, h, :M])).double()
        out.append(torch.as_tensor(q[b, :T, j]).double() @ k.T / 8)
    return torch.stack(out).numpy()


def reference(case, q, keys, b):
    """x of chunk b [n + 1][M] in f64: find_alignment steps 2-5 one head at a time (the mean over heads is linear)"""
    _, hk, S, width, qk_scale, chunks = case
    heads = HEADS[hk][2]
    n, nf = chunks[b]
    qk = head_scores(q, keys, heads, b, S + n + 2, nf // 2)
    return sum(alignment_matrix(qk[j:j + 1], S, nf, width, qk_scale, dtype=np.float64) for j in range(len(heads))) / len(heads)


def run_kernels(kctx, case, q, keys, col_stats=False):
    _, hk, S, width, qk_scale, chunks = case
    return kctx.align_matrix(q, keys, HEADS[hk][2], S, [n for n, _ in chunks], [nf for _, nf in chunks], width, qk_scale,
                             col_stats=col_stats)


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    out = os.environ.get("WM_MEASURED_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "align_kernels_measured.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def kctx(pkg):
    c = pkg.binding.Context(debug=True)   # no model: the hooks stage their own buffers
    yield c
    c.close()


def check_extent(x, chunks, label):
    """x is written on rows [0, n + 1) x frames [0, M) of every chunk and nowhere else (the sentinel survives)"""
    bits = x.view(np.uint32)
    for b, (n, nf) in enumerate(chunks):
        written = np.zeros(x.shape[1:], dtype=bool)
        if n > 0:
            written[:n + 1, :nf // 2] = True
        assert np.all(bits[b][~written] == SENTINEL), (label, b, "write outside the extent")
        assert not np.any(bits[b][written] == SENTINEL), (label, b, "cell of the extent not written")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cost_matrix_against_fp64(kctx, case):
    regime, hk, S, width, qk_scale, chunks = case
    q, keys = inputs(case, CASES.index(case))
    x, cs = run_kernels(kctx, case, q, keys, col_stats=True)
    label = case_id(case)
    check_extent(x, chunks, label)
    for b, (n, nf) in enumerate(chunks):
        M = nf // 2
        if M == 1:
            continue    # one frame: every column has zero spread (torch: nan), out of scope
        got, want = x[b, :n + 1, :M], reference(case, q, keys, b)
        assert np.all(np.isfinite(want)), (label, b)
        assert np.all(np.isfinite(got)), (label, b, int(np.sum(~np.isfinite(got))), "non-finite cells")
        e = float(np.abs(got - want).max())
        _note("x_" + regime, e)
        _note("x_%s_w%d" % (regime, width), e)
        # the column statistics behind x (informative: the x gate is the assertion)
        T = S + n + 2
        p = torch.softmax(torch.as_tensor(head_scores(q, keys, HEADS[hk][2], b, T, M)) * qk_scale, -1)
        sd, mean = torch.std_mean(p, dim=1, unbiased=False)
        _note("std_rel_" + regime, (np.abs(cs[b, :, :M, 1] - sd.numpy()) / sd.numpy()).max())
        _note("mean_rel_" + regime, (np.abs(cs[b, :, :M, 0] - mean.numpy()) / mean.numpy()).max())
        assert e <= GATES[regime], (label, b, n, M, e)


def test_batch_mixed_chunks_bit_identical_alone(kctx):
    """one batch of mixed n / M (an n_text = 0 chunk stays untouched); each chunk alone -- its own Tq, a one-chunk cache --
    gives the same bits as inside the batch"""
    case = ("normal", "three", 3, 7, 1.0, [(17, 3000), (0, 3000), (63, 1001), (1, 64), (16, 129), (64, 2)])
    q, keys = inputs(case, 101)
    x = run_kernels(kctx, case, q, keys)
    check_extent(x, case[5], "batch")
    for b, (n, nf) in enumerate(case[5]):
        if n == 0:
            continue
        alone = case[:5] + ([(n, nf)],)
        xa = run_kernels(kctx, alone, q[b:b + 1, :case[2] + n + 2], keys[:, b:b + 1])
        check_extent(xa, alone[5], "alone %d" % b)
        M = nf // 2
        assert np.array_equal(xa[0, :n + 1, :M].view(np.uint32), x[b, :n + 1, :M].view(np.uint32)), b
        if M > 1:
            assert np.abs(x[b, :n + 1, :M] - reference(case, q, keys, b)).max() <= GATES["normal"], b


def test_invalid_arguments_rejected(kctx, pkg):
    case = ("normal", "one", 1, 7, 1.0, [(3, 100)])
    q, keys = inputs(case, 0)
    heads = HEADS["one"][2]
    for kw in (dict(medfilt_width=8), dict(medfilt_width=33), dict(medfilt_width=-1), dict(n_text=4), dict(n_text=-1),
               dict(n_frames=1), dict(n_frames=3001), dict(qk_scale=float("nan")), dict(heads=[(2, 0)]),
               dict(heads=[(0, 3)])):
        a = dict(heads=heads, S=1, n_text=3, n_frames=100, medfilt_width=7, qk_scale=1.0)
        a.update(kw)
        with pytest.raises(pkg.binding.WhisperError) as e:
            kctx.align_matrix(q, keys, **a)
        assert e.value.status == 1, kw


@pytest.mark.parametrize("eot", [1, 255, 256, 257, 50257, 51865])
def test_token_prob_against_fp64(kctx, eot):
    """softmax(row[0 : eot])[tok]: tokens 0 and eot - 1, rows with a +-80 logit spread (underflowing probabilities), a
    probability ~1e-20, equal logits; row stride ldo > V; logits at eot and past V poisoned (never read)"""
    rng = np.random.default_rng(eot)
    V = eot + 3
    ldo = V + 37
    rows, toks = [], []
    for kind in ("normal", "normal", "spread-max", "spread-min", "spread", "tiny", "flat"):
        r = rng.standard_normal(eot) * 4
        tok = int(rng.integers(0, eot))
        if kind.startswith("spread"):
            r = rng.uniform(-80, 80, size=eot)
            tok = int(np.argmax(r)) if kind == "spread-max" else int(np.argmin(r)) if kind == "spread-min" else tok
        elif kind == "tiny":
            r[tok] = r.max() - 45.0 if eot > 1 else r[tok]
        elif kind == "flat":
            r[:] = 3.0
        rows.append(r)
        toks.append(tok)
    toks[0], toks[1] = 0, eot - 1
    logits = np.full((len(rows), ldo), np.nan, dtype=np.float32)
    logits[:, eot:V] = 1e4
    logits[:, :eot] = np.stack(rows)
    got = kctx.align_token_prob(logits, toks, eot, V=V)
    want = torch.softmax(torch.as_tensor(logits[:, :eot]).double(), -1).numpy()[np.arange(len(rows)), toks]
    err = np.abs(got.astype(np.float64) - want)
    big = want > 1e-30
    if big.any():
        _note("token_prob_rel", (err[big] / want[big]).max())
    assert np.all(err <= 1e-5 * want + 1e-30), (eot, got, want)     # measured: relative 1.9e-6
    if eot == 1:
        assert np.all(got == 1.0)
