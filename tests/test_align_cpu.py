"""CPU tests of word-level timestamps (wm_align): the numpy restatement of openai-whisper's find_alignment post-processing
(whisper/timing.py: z-score, median_filter, dtw_cpu in f32, backtrace, jump times) on hand-worked matrices, the host build
of csrc/dtw.h (the DTW cell rule and backtrace move the GPU kernel runs) against that restatement, and
binding.word_timestamps (split_to_word_tokens + merge_punctuations) on a synthetic vocab.json.  The GPU side is
tests/test_align_gpu.py, which imports the restatement from here."""
import ctypes
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

B = importlib.import_module("openai_whisper_coreml_amd.binding")


# ---------------------------------------------------------------- numpy / torch restatement
def median_filter(x, width, dtype=np.float32):
    """openai-whisper median_filter: along the last axis, reflect padding of width // 2, none when it would not fit."""
    x = torch.as_tensor(np.asarray(x, dtype=dtype))
    pad = width // 2
    if x.shape[-1] <= pad:
        return x.numpy()
    nd = x.ndim
    y = x[None, None] if nd <= 2 else x
    y = F.pad(y, (pad, pad, 0, 0), mode="reflect")
    r = y.unfold(-1, width, 1).sort()[0][..., pad]
    return (r[0, 0] if nd <= 2 else r).numpy()


def zscore(w, dtype=np.float32):
    """per head and frame over the rows (torch.std_mean(dim=-2, unbiased=False))"""
    w = torch.as_tensor(np.asarray(w, dtype=dtype))
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    return ((w - mean) / std).numpy()


def dtw_trace(x):
    """openai-whisper dtw_cpu in f32: cost[0][0] = 0, other borders +inf, its tie rule; walked along the anti-diagonals
    (the cells of one diagonal do not depend on each other)."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    cost[0, 0] = 0
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c          # one f32 add
        trace[i, j] = t
    return trace


def backtrace(trace):
    """openai-whisper backtrace -> (text_indices, time_indices)"""
    trace = trace.copy()
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace[0, :] = 2
    trace[:, 0] = 1
    res = []
    while i > 0 or j > 0:
        res.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            raise ValueError("unexpected trace")
    res = np.array(res)[::-1]
    return res[:, 0], res[:, 1]


def start_frames(x):
    """find_alignment's jump_times * 50: the first frame of every row of x on the DTW path."""
    text_idx, time_idx = backtrace(dtw_trace(x))
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    return time_idx[jumps].astype(np.int64)


def alignment_matrix(qk, n_sot, n_frames, medfilt_width=7, qk_scale=1.0, dtype=np.float32):
    """find_alignment steps 2-5 on the recorded scores of the alignment heads, qk [J][T][>= n_frames // 2] (= q.k / 8), in
    `dtype` throughout (openai-whisper: f32): the cost matrix -matrix [n + 1][n_frames // 2]."""
    w = torch.as_tensor(np.asarray(qk, dtype=dtype))[:, :, : n_frames // 2]
    w = (w * qk_scale).softmax(dim=-1).numpy()
    w = median_filter(zscore(w, dtype), medfilt_width, dtype)
    matrix = np.asarray(w).mean(axis=0)
    return -matrix[n_sot:-1]


def _variant_matrix(qk, n_sot, n_frames, medfilt_width, qk_scale, variant):
    """alignment_matrix in f64 for one head with one deliberate mistake ("none": without): "unbiased" std (ddof 1), "shifted" median window
    (frames fo - h + 1 .. fo + h + 1), "replicate" padding, "text-rows" (the column statistics over the n + 1 text rows
    only, not all S + n + 2 rows)."""
    w = (torch.as_tensor(np.asarray(qk, dtype=np.float64))[:, :, : n_frames // 2] * qk_scale).softmax(dim=-1)
    rows = w[:, n_sot:-1] if variant == "text-rows" else w
    std, mean = torch.std_mean(rows, dim=-2, keepdim=True, unbiased=variant == "unbiased")
    z = (w - mean) / std
    h, M = medfilt_width // 2, w.shape[-1]
    if M > h + (variant == "shifted"):
        y = F.pad(z, (h, h + (variant == "shifted"), 0, 0), mode="replicate" if variant == "replicate" else "reflect")
        z = y.unfold(-1, medfilt_width, 1).sort()[0][..., h][..., variant == "shifted":][..., :M]
    return -z.mean(dim=0).numpy()[n_sot:-1]


# ---------------------------------------------------------------- hand-worked cases
def test_median_filter_and_zscore_by_hand():
    x = np.array([[5, 1, 4, 2, 3, 9, 0]], dtype=np.float32)
    # reflect padding: [4, 1, | 5 1 4 2 3 9 0 | 9, 3]; width 3 -> medians of (1 5 1) (5 1 4) (1 4 2) (4 2 3) (2 3 9) (3 9 0) (9 0 9)
    assert median_filter(x, 3).tolist() == [[1, 4, 2, 3, 3, 3, 9]]
    assert median_filter(x, 1).tolist() == x.tolist()
    assert median_filter(x[:, :3], 7).tolist() == x[:, :3].tolist()   # 3 frames <= 7 // 2: no filtering
    w = np.array([[[1.0, 2.0], [3.0, 2.0]]], dtype=np.float32)      # one head, two rows, two frames
    z = zscore(w)
    assert np.allclose(z[0, :, 0], [-1, 1]) and np.all(np.isnan(z[0, :, 1]))   # zero spread: nan, as torch


@pytest.mark.parametrize("x, want", [
    (np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.float32), [0, 1, 2]),          # a diagonal
    (np.array([[0, 0, 1, 1], [1, 1, 0, 0]], dtype=np.float32), [0, 2]),                  # a staircase
    (np.zeros((2, 3), dtype=np.float32), [0, 0]),                                        # all ties: left, then up
    (np.zeros((3, 1), dtype=np.float32), [0, 0, 0]),                                     # one frame
    (np.array([[3, 2, 1, 0]], dtype=np.float32), [0]),                                   # one row
])
def test_dtw_and_backtrace_by_hand(x, want):
    assert start_frames(x).tolist() == want


def test_tie_rule_prefers_the_left_cell_over_a_tied_diagonal():
    """cell (2, 2) of the staircase: c0 = c1 = 0 < c2 = 1, yet neither is strictly smallest -> c2 (openai-whisper's rule)"""
    tr = dtw_trace(np.array([[0, 0, 1, 1], [1, 1, 0, 0]], dtype=np.float32))
    assert tr[2, 2] == 2 and tr[2, 3] == 0 and tr[1, 1] == 0


# ---------------------------------------------------------------- the host build of csrc/dtw.h
_SHIM = r"""
#include <stdlib.h>
#include "dtw.h"
extern "C" void shim_dtw(const float *x, int N, int M, int *start) {
    float *cost = (float *)malloc(sizeof(float) * (N + 1) * (M + 1));
    unsigned char *tr = (unsigned char *)malloc((size_t)(N + 1) * (M + 1));
    const float inf = __builtin_inff();
    for (int i = 0; i <= N; ++i)
        for (int j = 0; j <= M; ++j) cost[i * (M + 1) + j] = (i == 0 && j == 0) ? 0.f : inf;
    for (int j = 1; j <= M; ++j)
        for (int i = 1; i <= N; ++i) {
            int t;
            cost[i * (M + 1) + j] = wm_dtw_cell(x[(i - 1) * M + j - 1], cost[(i - 1) * (M + 1) + j - 1],
                                                cost[(i - 1) * (M + 1) + j], cost[i * (M + 1) + j - 1], &t);
            tr[i * (M + 1) + j] = (unsigned char)t;
        }
    int i = N, j = M;
    while (i > 0 || j > 0) {
        const int t = i == 0 ? 2 : j == 0 ? 1 : tr[i * (M + 1) + j];
        int row, frame;
        wm_dtw_move(t, &i, &j, &row, &frame);
        if (row >= 0) start[row] = frame;
    }
    free(cost);
    free(tr);
}
"""


@pytest.fixture(scope="module")
def host_dtw(tmp_path_factory):
    """csrc/dtw.h compiled for the HOST (the same header the DTW kernel includes), column-major like dtw_cpu."""
    d = tmp_path_factory.mktemp("dtw")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(_SHIM)
    inc = os.path.join(ROOT, "openai-whisper-coreml_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", inc, str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    lib.shim_dtw.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.shim_dtw.restype = None

    def run(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.full(x.shape[0], -7, dtype=np.int32)
        lib.shim_dtw(x.ctypes.data_as(ctypes.c_void_p), x.shape[0], x.shape[1], out.ctypes.data_as(ctypes.c_void_p))
        return out
    return run


def test_host_build_of_the_cell_rule_matches_numpy(host_dtw):
    rng = np.random.default_rng(7)
    shapes = [(1, 1), (1, 5), (5, 1), (2, 3), (17, 40), (60, 200), (225, 300)]
    for n, m in shapes:
        for kind in ("random", "ties", "cumulative-ties"):
            if kind == "random":
                x = rng.standard_normal((n, m)).astype(np.float32)
            elif kind == "ties":                  # small integers: equal costs everywhere
                x = rng.integers(0, 3, size=(n, m)).astype(np.float32)
            else:                                 # integer z-score-like values: ties of the accumulated costs
                x = rng.integers(-2, 3, size=(n, m)).astype(np.float32)
            want = start_frames(x)
            got = host_dtw(x)
            assert got.tolist() == want.tolist(), (n, m, kind)


# ---------------------------------------------------------------- word_timestamps
def _bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + \
        list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


PIECES = [b" hello", b" wor", b"ld", b",", b" (", b" yes", b")", b".",
          "中".encode()[:2], "中".encode()[2:], b" caf", "é".encode()[:1], "é".encode()[1:],
          "文".encode(), "字".encode()]


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    b2u = _bytes_to_unicode()
    path = tmp_path_factory.mktemp("vocab") / "vocab.json"
    path.write_text(json.dumps({"".join(b2u[c] for c in p): i for i, p in enumerate(PIECES)}), encoding="utf-8")
    v = B.Vocab(str(path))
    yield v
    v.close()


def test_words_spaces_and_punctuation(vocab):
    toks = [0, 1, 2, 3, 4, 5, 6, 7]
    sf = np.array([0, 10, 20, 30, 40, 50, 60, 70, 80])
    pr = np.array([0.9, 0.5, 0.7, 0.8, 0.6, 0.4, 0.3, 0.2], dtype=np.float32)
    words = B.word_timestamps(vocab, toks, sf, pr)
    assert [w["word"] for w in words] == [" hello", " world,", " ( yes)."]
    assert [w["tokens"] for w in words] == [[0], [1, 2, 3], [4, 5, 6, 7]]
    # merged punctuation keeps the word's own times and probability (openai-whisper merge_punctuations)
    assert [(w["start"], w["end"]) for w in words] == [(0.0, 0.2), (0.2, 0.6), (1.0, 1.2)]
    assert np.allclose([w["probability"] for w in words], [0.9, np.mean(pr[1:3]), pr[5]])


def test_words_multibyte_piece_split_across_tokens(vocab):
    toks = [10, 11, 12, 1, 2]          # " caf" + the two bytes of e-acute, " wor" + "ld"
    sf = np.array([3, 5, 9, 11, 14, 20])
    pr = np.array([0.5, 0.25, 1.0, 0.5, 0.5], dtype=np.float32)
    words = B.word_timestamps(vocab, toks, sf, pr)
    assert [w["word"] for w in words] == [" café", " world"]
    assert [w["tokens"] for w in words] == [[10, 11, 12], [1, 2]]
    assert [(w["start"], w["end"]) for w in words] == [(3 / 50, 11 / 50), (11 / 50, 20 / 50)]
    assert np.allclose([w["probability"] for w in words], [np.mean(pr[:3]), 0.5])


def test_words_no_space_language(vocab):
    toks = [8, 9, 13, 14, 3]           # the character 中 split over two tokens, then 文, 字 and ","
    sf = np.array([0, 4, 8, 12, 16, 17])
    pr = np.array([0.2, 0.4, 0.6, 0.8, 1.0], dtype=np.float32)
    words = B.word_timestamps(vocab, toks, sf, pr, language="zh")
    assert [w["word"] for w in words] == ["中", "文", "字,"]
    assert [w["tokens"] for w in words] == [[8, 9], [13], [14, 3]]
    assert [(w["start"], w["end"]) for w in words] == [(0.0, 8 / 50), (8 / 50, 12 / 50), (12 / 50, 16 / 50)]
    # the same tokens under the space rule: one word (no space anywhere), then the comma appended
    words_en = B.word_timestamps(vocab, toks, sf, pr, language="en")
    assert [w["word"] for w in words_en] == ["中文字,"]


def test_words_edge_cases(vocab):
    assert B.word_timestamps(vocab, [], np.array([-1]), np.zeros(0)) == []
    w = B.word_timestamps(vocab, [0], np.array([2, 7]), np.array([0.5]))
    assert w == [dict(word=" hello", tokens=[0], start=2 / 50, end=7 / 50, probability=0.5)]


# ---------------------------------------------------------------- the fp64 reference of tests/test_align_kernels_gpu.py
def test_fp64_restatement_matches_the_f32_one():
    """well-conditioned scores (q, k ~ N(0, 1)): the fp64 restatement the kernel tests use and the f32 one agree to within
    the kernel tests' gate for such inputs"""
    K = importlib.import_module("test_align_kernels_gpu")
    rng = np.random.default_rng(1)
    for T, M, width in ((5, 2, 3), (20, 64, 7), (60, 617, 15), (448, 1500, 31)):
        qk = rng.standard_normal((3, T, 64)) @ rng.standard_normal((M, 64)).T / 8
        x64 = alignment_matrix(qk, 3, 2 * M, width, 0.37, dtype=np.float64)
        x32 = alignment_matrix(qk, 3, 2 * M, width, 0.37)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and x64.shape == (T - 4, M)
        assert np.abs(x64 - x32).max() <= K.GATES["normal"], (T, M, width, np.abs(x64 - x32).max())


def test_kernel_gates_catch_known_wrong_variants():
    """On the kernel tests' own inputs (chunks of up to 64 text tokens), each known-wrong variant moves x by more than 10x the
    regime's gate in some case of every regime: the gates would catch a kernel that made that mistake."""
    K = importlib.import_module("test_align_kernels_gpu")
    worst = {}
    for i, case in enumerate(K.CASES):
        regime, hk, S, width, qk_scale, chunks = case
        heads = K.HEADS[hk][2]
        q, keys = K.inputs(case, i)
        for b, (n, nf) in enumerate(chunks):
            if n > 64 or nf // 2 < 2:
                continue
            qk = K.head_scores(q, keys, heads, b, S + n + 2, nf // 2)
            want = K.reference(case, q, keys, b)
            for variant in ("none", "unbiased", "shifted", "replicate", "text-rows"):
                got = np.mean([_variant_matrix(qk[j:j + 1], S, nf, width, qk_scale, variant) for j in range(len(heads))], 0)
                d = np.abs(got - want).max() / K.GATES[regime]
                if variant == "none":
                    assert d <= 1e-6, (K.case_id(case), b)    # without a mistake: the reference itself
                    continue
                worst[variant, regime] = max(worst.get((variant, regime), 0.0), d)
    assert len(worst) == 4 * len(K.GATES)
    weak = {k: v for k, v in worst.items() if not v > 10}
    assert not weak, weak
