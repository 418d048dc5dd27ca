"""GPU unit tests of the alignment kernels' row rule for an aligned transcribe group (csrc/align.hip, WmAlignDev::tail = 0)
through wmdbg_align_matrix_rows: a chunk of S + N decoder rows whose cost matrix is the LAST N of them -- no row behind the
last matrix row, a one-row matrix allowed -- against the f64 restatement of tests/test_align_kernels_gpu.py on the same f32
queries and bf16-rounded keys.  Inputs q, k ~ N(0, 1) (that file's "normal" regime) and its bound for them."""
import numpy as np
import pytest
import torch

from test_align_cpu import median_filter, zscore
from test_align_kernels_gpu import GATES, HEADS, SENTINEL, head_scores, kctx  # noqa: F401  (kctx: module fixture)

pytestmark = pytest.mark.gpu

L, H, HEADS3 = HEADS["three"]      # J = 3
ROWS = (1, 2, 37)                  # matrix rows: one row, two, and three 16-row tiles with a ragged last one
FRAMES = (3, 64, 617)              # M: narrower than the filter's half-width + 1, one 64-frame tile exactly, ten tiles less 23


def _inputs(S, chunks, seed):
    """(q f32 [B][Tq][J][64], keys f32 [L][B][H][1500][64]) as test_align_kernels_gpu.inputs: q rows past a chunk's S + N and
    the keys of every head that is no alignment head are NaN -- the kernels must never read them"""
    B, J = len(chunks), len(HEADS3)
    Tq = S + max(n for n, _ in chunks)
    rng = np.random.default_rng(seed)
    keys = np.full((L, B, H, 1500, 64), np.nan, dtype=np.float32)
    q = np.full((B, Tq, J, 64), np.nan, dtype=np.float32)
    for b, (n, _) in enumerate(chunks):
        for j, (l, h) in enumerate(HEADS3):
            keys[l, b, h] = rng.standard_normal((1500, 64))
            q[b, :S + n, j] = rng.standard_normal((S + n, 64))
    return q, keys


def _reference(q, keys, b, S, n, nf, width):
    """x of chunk b [n][M] in f64: softmax, z-score over all S + n rows, median filter, -mean over the heads, the last n rows"""
    qk = head_scores(q, keys, HEADS3, b, S + n, nf // 2)
    w = torch.as_tensor(qk).softmax(dim=-1).numpy()
    w = median_filter(zscore(w, np.float64), width, np.float64)
    return -np.asarray(w).mean(axis=0)[S:]


def _check_extent(x, chunks):
    bits = x.view(np.uint32)
    for b, (n, nf) in enumerate(chunks):
        written = np.zeros(x.shape[1:], dtype=bool)
        written[:n, :nf // 2] = True
        assert np.all(bits[b][~written] == SENTINEL), (b, "write outside the extent")
        assert not np.any(bits[b][written] == SENTINEL), (b, "cell of the extent not written")


@pytest.mark.parametrize("width", [1, 7])
@pytest.mark.parametrize("S", [2, 0])
def test_row_rule_against_fp64(kctx, S, width):
    """every (rows, M) pair in one batch; S = 0 (a prompt that ends in <|startoftranscript|>) leaves out the one-row chunk,
    whose single decoder row has no spread.  A chunk of TWO decoder rows (S = 0, 2 rows) is not the "normal" regime: over two
    rows z = (p - mean) / std is +-1 by construction and p - mean = (p0 - p1) / 2 cancels, so a cell's error is
    ~ eps_f32 * p / |p0 - p1|, and among its J * M <= 1851 (head, frame) pairs the closest pair of N(0, 1)-scored
    probabilities differs by ~1e-3 relative: the per-frame coefficient of variation of that file's "cv1e-3" regime, whose gate
    applies to it."""
    chunks = [(n, 2 * m + (n & 1)) for n in ROWS for m in FRAMES if S + n >= 2]
    q, keys = _inputs(S, chunks, 100 * S + width)
    x = kctx.align_matrix_rows(q, keys, HEADS3, S, [n - 1 for n, _ in chunks], [nf for _, nf in chunks], width, 1.0, tail_rows=0)
    assert x.shape == (len(chunks), max(n for n, _ in chunks), 1500)
    _check_extent(x, chunks)
    worst = 0.0
    for b, (n, nf) in enumerate(chunks):
        got, want = x[b, :n, :nf // 2], _reference(q, keys, b, S, n, nf, width)
        assert want.shape == got.shape and np.all(np.isfinite(want)) and np.all(np.isfinite(got)), (b, n, nf)
        e = float(np.abs(got - want).max())
        worst = max(worst, e)
        assert e <= GATES["cv1e-3" if S + n == 2 else "normal"], (S, width, b, n, nf // 2, e)
    print("row rule S=%d width=%d: max|x - x_ref| %.3g (gate %.1g)" % (S, width, worst, GATES["normal"]))


def test_absent_chunks_stay_untouched_and_a_chunk_alone_has_the_batch_s_bits(kctx):
    S, width = 2, 7
    chunks = [(37, 1234), (0, 3000), (1, 128), (2, 7)]      # (0 rows: n_text -1, the absent chunk)
    q, keys = _inputs(S, chunks, 9)
    x = kctx.align_matrix_rows(q, keys, HEADS3, S, [n - 1 for n, _ in chunks], [nf for _, nf in chunks], width, 1.0)
    _check_extent(x, chunks)
    for b, (n, nf) in enumerate(chunks):
        if n == 0:
            continue
        xa = kctx.align_matrix_rows(q[b:b + 1, :S + n], keys[:, b:b + 1], HEADS3, S, [n - 1], [nf], width, 1.0)
        assert np.array_equal(xa[0, :n, :nf // 2].view(np.uint32), x[b, :n, :nf // 2].view(np.uint32)), b


def test_tail_row_one_is_the_existing_hook_and_bad_row_counts_are_rejected(kctx, pkg):
    S, n, nf = 3, 17, 258
    rng = np.random.default_rng(5)
    q = rng.standard_normal((1, S + n + 2, 3, 64)).astype(np.float32)
    keys = np.full((L, 1, H, 1500, 64), np.nan, dtype=np.float32)
    for l, h in HEADS3:
        keys[l, 0, h] = rng.standard_normal((1500, 64))
    old = kctx.align_matrix(q, keys, HEADS3, S, [n], [nf], 7, 1.0)
    new = kctx.align_matrix_rows(q, keys, HEADS3, S, [n], [nf], 7, 1.0, tail_rows=1)
    assert np.array_equal(old.view(np.uint32), new.view(np.uint32))
    for kw in (dict(tail_rows=2), dict(tail_rows=-1), dict(n_text=[-2]), dict(n_text=[S + n + 2 - S]), dict(S=0, n_text=[0]),
               dict(S=-1)):
        a = dict(S=S, n_text=[n], tail_rows=0)
        a.update(kw)
        with pytest.raises(pkg.binding.WhisperError) as e:
            kctx.align_matrix_rows(q, keys, HEADS3, a["S"], a["n_text"], [nf], 7, 1.0, tail_rows=a["tail_rows"])
        assert e.value.status == 1, kw
