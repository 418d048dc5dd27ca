"""CPU tests of wm_transcribe's host-checkable parts: the Philox-4x32-10 stream and the Gumbel map of its temperature
sampling (csrc/philox.h, built for the host here, against a numpy restatement and the Random123 known-answer vectors), and
the decision logic of Context.transcribe_with_fallback (openai-whisper's decode_with_fallback) against a scripted context.
The GPU side is tests/test_transcribe_options_gpu.py."""
import ctypes
import importlib
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT

B = importlib.import_module("openai_whisper_coreml_amd.binding")

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox_np(ctr, key):
    """Philox-4x32-10 over arrays: ctr uint32 [..., 4], key (k0, k1) -> uint32 [..., 4]."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, axis=-1).astype(np.uint32)


def sample_bits_np(seed, chunk, gi, n):
    """The 32-bit draw of token ids n (array) at generated index gi of chunk `chunk` (csrc/philox.h wm_sample_bits)."""
    n = np.asarray(n, dtype=np.uint64)
    ctr = np.stack([n >> np.uint64(2), np.full_like(n, gi), np.full_like(n, chunk), np.zeros_like(n)], axis=-1)
    out = philox_np(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return np.take_along_axis(out, (n & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def uniform_np(x):
    """u = ((x >> 9) * 2 + 1) * 2^-24 (exact in f32 and f64)."""
    return (((np.asarray(x, dtype=np.uint64) >> np.uint64(9)) * np.uint64(2) + np.uint64(1)).astype(np.float64)) * 2.0 ** -24


def gumbel_np(seed, chunk, gi, n):
    """g(n) = -log(-log u(n)) in float64: the noise wm_transcribe adds to logit / T."""
    u = uniform_np(sample_bits_np(seed, chunk, gi, n))
    return -np.log(-np.log(u))


# Random123 kat_vectors (philox4x32, 10 rounds): counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_numpy_philox_reproduces_the_random123_vectors():
    for ctr, key, want in KAT:
        got = philox_np(np.array(ctr, dtype=np.uint32)[None], key)[0]
        assert [int(v) for v in got] == list(want), (ctr, key, ["%08x" % v for v in got])


_SHIM = r"""
#include "philox.h"
extern "C" {
void shim_philox(const uint32_t *ctr, uint32_t k0, uint32_t k1, uint32_t *out, int n) {
    for (int i = 0; i < n; ++i) {
        wm_philox4 c;
        for (int j = 0; j < 4; ++j) c.v[j] = ctr[4 * i + j];
        const wm_philox4 r = wm_philox4x32_10(c, k0, k1);
        for (int j = 0; j < 4; ++j) out[4 * i + j] = r.v[j];
    }
}
void shim_bits(uint64_t seed, uint32_t chunk, uint32_t gi, uint32_t n0, int count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = wm_sample_bits(seed, chunk, gi, n0 + (uint32_t)i);
}
void shim_uniform(const uint32_t *x, int n, float *u, float *g) {
    for (int i = 0; i < n; ++i) { u[i] = wm_uniform_from_bits(x[i]); g[i] = wm_gumbel_from_bits(x[i]); }
}
}
"""


@pytest.fixture(scope="module")
def host_philox(tmp_path_factory):
    """csrc/philox.h compiled for the HOST (the same header the decode kernels include)."""
    d = tmp_path_factory.mktemp("philox")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(_SHIM)
    inc = os.path.join(ROOT, "openai-whisper-coreml_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I", inc, str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    vp = ctypes.c_void_p
    lib.shim_philox.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_int]
    lib.shim_bits.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, vp]
    lib.shim_uniform.argtypes = [vp, ctypes.c_int, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_host_build_of_the_header_matches_numpy(host_philox):
    for ctr, key, want in KAT:
        c = np.array(ctr, dtype=np.uint32)
        out = np.zeros(4, dtype=np.uint32)
        host_philox.shim_philox(_p(c), key[0], key[1], _p(out), 1)
        assert [int(v) for v in out] == list(want)
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32)
    for key in ((0, 0), (0x12345678, 0x9abcdef0), (0xffffffff, 1)):
        out = np.zeros_like(ctr)
        host_philox.shim_philox(_p(np.ascontiguousarray(ctr)), key[0], key[1], _p(out), len(ctr))
        assert np.array_equal(out, philox_np(ctr, key))
    # the token-id stream: counter {n >> 2, gi, chunk, 0}, word n & 3, key = the seed's two halves
    for seed, chunk, gi in ((0, 0, 0), (2 ** 40 + 12345, 17, 3), (2 ** 64 - 1, 127, 447)):
        n0, cnt = 51000, 866
        bits = np.zeros(cnt, dtype=np.uint32)
        host_philox.shim_bits(seed, chunk, gi, n0, cnt, _p(bits))
        assert np.array_equal(bits, sample_bits_np(seed, chunk, gi, np.arange(n0, n0 + cnt)))


def test_uniform_and_gumbel_maps_are_exact_and_finite_at_the_extremes(host_philox):
    x = np.array([0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff] +
                 list(np.random.default_rng(3).integers(0, 2 ** 32, 4096)), dtype=np.uint32)
    u = np.zeros(len(x), dtype=np.float32)
    g = np.zeros(len(x), dtype=np.float32)
    host_philox.shim_uniform(_p(x), len(x), _p(u), _p(g))
    want_u = uniform_np(x)
    assert np.array_equal(u.astype(np.float64), want_u)        # exact: odd multiples of 2^-24 below 1
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    assert np.all((u > 0) & (u < 1))
    assert np.all(np.isfinite(g))
    want_g = -np.log(-np.log(want_u))
    # the header's f32 map (log1p-like series near u = 1) stays within a few f32 ulps of the f64 value
    assert np.max(np.abs(g - want_g) / np.maximum(1.0, np.abs(want_g))) < 2e-6
    assert abs(float(g[0]) - (-np.log(-np.log(2.0 ** -24)))) < 1e-5          # x = 0: g = -2.81
    assert abs(float(g[7]) - (-np.log(-np.log1p(-2.0 ** -24)))) < 1e-5       # x = 2^32 - 1: g = 16.64


# ------------------------------------------------------------------ temperature fallback (decision logic)
class ScriptedContext:
    """Stands in for Context.transcribe: per (temperature, chunk id) a scripted (tokens, logprob per token, no_speech);
    records every call.  Chunk ids are carried in the pcm rows."""

    def __init__(self, script, max_new, eot, n_vocab=1024):
        self.script, self.eot, self.calls = script, eot, []
        self.max_new = max_new
        self.dims = {"n_vocab": n_vocab}

    def transcribe(self, pcm, prompt, max_new, eot=-1, temperature=0.0, seed=0, no_speech_token=-1, sot_index=0):
        ids = [int(r[0]) for r in pcm]
        self.calls.append((temperature, seed, ids))
        n = len(ids)
        toks = np.full((n, max_new), eot, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        lp = np.zeros((n, max_new), dtype=np.float32)
        ns = np.zeros(n, dtype=np.float32)
        for i, c in enumerate(ids):
            t, l, p = self.script[(temperature, c)]
            toks[i, :len(t)] = t
            lens[i] = len(t)
            lp[i, :len(t)] = l
            ns[i] = p
        return B.TranscribeResult(toks, lens, lp, ns if no_speech_token >= 0 else None, eot)


def _pcm(n):
    return np.arange(n, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)


def test_fallback_redecodes_only_failing_chunks_in_one_call_per_temperature():
    EOT = 99
    good = ([5, 6, 7, EOT], [-0.1] * 4)          # avg = -0.4 / 4
    bad_lp = ([5, 6, 7, EOT], [-2.0] * 4)        # avg = -8 / 4 = -2 < -1
    loop = ([5] * 40 + [EOT], [-0.1] * 41)       # a repetition loop: compression ratio far above the threshold
    script = {}
    # chunk 0: fine at T=0.  chunk 1: low log-prob until 0.4.  chunk 2: repetition until 0.2.  chunk 3: low log-prob,
    # but no_speech_prob above the threshold -> no fallback.  chunk 4: fails at every temperature -> keeps the last.
    for T in B.FALLBACK_TEMPERATURES:
        script[(T, 0)] = good + (0.1,)
        script[(T, 1)] = (bad_lp if T < 0.4 else good) + (0.1,)
        script[(T, 2)] = (loop if T < 0.2 else good) + (0.1,)
        script[(T, 3)] = bad_lp + (0.9,)
        script[(T, 4)] = ([5, 6, 7 + int(10 * T), EOT], [-3.0] * 4, 0.1)
    ctx = ScriptedContext(script, 48, EOT)
    r = B.transcribe_with_fallback(ctx, _pcm(5), [1], 48, EOT, seed=100, no_speech_token=98)
    calls = [(t, s, ids) for t, s, ids in ctx.calls]
    assert calls == [(0.0, 100, [0, 1, 2, 3, 4]), (0.2, 101, [1, 2, 4]), (0.4, 102, [1, 4]), (0.6, 103, [4]),
                     (0.8, 104, [4]), (1.0, 105, [4])]
    assert [s[0] for s in r["steps"]] == list(B.FALLBACK_TEMPERATURES)
    assert list(r["temperature"]) == [0.0, 0.4, 0.2, 0.0, 1.0]
    assert list(r["seed"]) == [100, 102, 101, 100, 105]
    assert list(r["needs_fallback"]) == [False, False, False, False, True]
    assert r["tokens"][4, 2] == 17                      # the last result is kept
    assert r["avg_logprob"][0] == pytest.approx(-0.4 / 4) and r["avg_logprob"][4] == pytest.approx(-12.0 / 4)
    assert r["no_speech_prob"][3] == pytest.approx(0.9)
    # without a no-speech token the override is off: chunk 3 falls back to the end
    ctx = ScriptedContext(script, 48, EOT)
    r = B.transcribe_with_fallback(ctx, _pcm(5), [1], 48, EOT, seed=0)
    assert ctx.calls[1][2] == [1, 2, 3, 4] and list(r["temperature"])[3] == 1.0
    # thresholds switched off (None): nothing falls back
    ctx = ScriptedContext(script, 48, EOT)
    B.transcribe_with_fallback(ctx, _pcm(5), [1], 48, EOT, logprob_threshold=None, compression_ratio_threshold=None)
    assert len(ctx.calls) == 1
    # only the compression ratio switched off: the low log-prob chunks still fall back, the repetition loop does not
    ctx = ScriptedContext(script, 48, EOT)
    B.transcribe_with_fallback(ctx, _pcm(5), [1], 48, EOT, compression_ratio_threshold=None)
    assert ctx.calls[1][2] == [1, 3, 4]
    with pytest.raises(ValueError):
        B.transcribe_with_fallback(ctx, _pcm(5), [1], 48, EOT, compression_ratio_threshold="openai")


def test_avg_logprob_counts_text_tokens_plus_one():
    toks = np.array([[3, 4, 9, 9], [3, 4, 5, 6]], dtype=np.int32)
    lens = np.array([3, 4], dtype=np.int32)
    lp = np.array([[-1, -2, -3, 0], [-1, -1, -1, -1]], dtype=np.float32)
    r = B.TranscribeResult(toks, lens, lp, None, 9)
    assert list(r.sum_logprob) == [-6.0, -4.0]
    assert list(r.n_text) == [2, 4]                     # chunk 1 hit its budget: no eot, every token is text
    assert r.avg_logprob[0] == pytest.approx(-6.0 / 3) and r.avg_logprob[1] == pytest.approx(-4.0 / 5)


def test_compression_ratio_rules_by_hand():
    # openai-whisper: len(utf8) / len(zlib(utf8))
    text = "the cat " * 20
    b = text.encode()
    assert B.compression_ratio_text(text) == len(b) / len(zlib.compress(b)) == 160 / len(zlib.compress(b))
    assert B.compression_ratio_text("héllo") == 6 / len(zlib.compress("héllo".encode()))
    # transformers: int(log2(51865) / 8) + 1 = 2 bytes per id, little-endian
    toks = [50364, 1, 258]
    raw = bytes([0xBC, 0xC4, 0x01, 0x00, 0x02, 0x01])
    assert B.compression_ratio_tokens(toks, 51865) == 6 / len(zlib.compress(raw))
    # a tiny vocabulary (1024): still 2 bytes (int(10 / 8) + 1); 256 ids: 2 bytes too (int(8 / 8) + 1)
    assert B.compression_ratio_tokens([1, 2], 1024) == 4 / len(zlib.compress(b"\x01\x00\x02\x00"))
    assert B.compression_ratio_tokens([7], 256) == 2 / len(zlib.compress(b"\x07\x00"))
    # with a vocabulary the helper uses the text rule (and its 2.4 default); without, the token rule (1.35)
    EOT = 99
    script = {(0.0, 0): ([5, 6, EOT], [-0.1] * 3, 0.0), (0.2, 0): ([5, EOT], [-0.1] * 2, 0.0)}

    class V:
        def decode(self, ids):
            return "the cat " * 20

    ctx = ScriptedContext(script, 8, EOT)
    r = B.transcribe_with_fallback(ctx, _pcm(1), [1], 8, EOT, temperatures=(0.0, 0.2), vocab=V())
    assert r["compression_ratio"][0] == pytest.approx(B.compression_ratio_text("the cat " * 20))
    assert r["temperature"][0] == 0.2                   # 160 / ~16 bytes > 2.4
    ctx = ScriptedContext(script, 8, EOT)
    r = B.transcribe_with_fallback(ctx, _pcm(1), [1], 8, EOT, temperatures=(0.0, 0.2))
    assert r["compression_ratio"][0] == pytest.approx(B.compression_ratio_tokens([5, 6], 1024))
    assert r["temperature"][0] == 0.0                   # 4 bytes compress to more than 4: ratio < 1.35


def test_header_declares_the_new_entry_points():
    h = open(os.path.join(ROOT, "include", "whisper_mi355x.h")).read()
    assert "WM_API int wm_transcribe(" in h and "typedef struct wm_decode_opts" in h
    dh = open(os.path.join(ROOT, "include", "whisper_mi355x_debug.h")).read()
    assert "wmdbg_sample_noise" in dh
