"""CPU tests of best-of-N sampling (include/whisper_mi355x.h wm_transcribe_mel_best_of, wm_rank_candidates): the host-only
ranker against a numpy restatement of openai-whisper's MaximumLikelihoodRanker, the pure decode-group cut of a candidate
call, the candidate word of the Philox counter (csrc/philox.h built for the host), transcribe_long(best_of=) on a fake
context, and an ISA lint of the candidate cross-attention kernel (cross-compiled, as tests/test_isa_cpu.py does it).

The ranker, restated (whisper/decoding.py, with this project's rule for a candidate without text):
    sum     = f64 sum of the candidate's token log-probs in index order (the stopping eot included)
    n_text  = tokens before the first eot
    penalty = n_text (1 when n_text == 0)             length_penalty None (NaN in the C ABI)
              ((5 + n_text) / 6) ** length_penalty    otherwise
    score   = sum / penalty; the first maximal score wins; every score -inf: candidate 0."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_ragged_prompts_cpu import EOT, FakeCtx, _fake_kw
from test_transcribe_options_cpu import philox_np, sample_bits_np

B = importlib.import_module("openai_whisper_coreml_amd.binding")


# ---------------------------------------------------------------- the ranker
def rank_np(tokens, lens, logprobs, eot, length_penalty):
    nB, N, _ = tokens.shape
    best = np.zeros(nB, np.int32)
    scores = np.zeros((nB, N))
    for b in range(nB):
        top = -np.inf
        for s in range(N):
            n = int(lens[b, s])
            total = 0.0
            for i in range(n):
                total += float(logprobs[b, s, i])
            hit = np.flatnonzero(tokens[b, s, :n] == eot)
            n_text = int(hit[0]) if hit.size else n
            if length_penalty is None:
                pen = float(n_text) if n_text > 0 else 1.0
            else:
                pen = ((5.0 + n_text) / 6.0) ** float(np.float32(length_penalty))   # (the C ABI takes an f32)
            scores[b, s] = total / pen
            if scores[b, s] > top:
                top, best[b] = scores[b, s], s
    return best, scores


def _random_candidates(rng, nB, N, max_new, eot):
    tokens = rng.integers(0, eot, size=(nB, N, max_new)).astype(np.int32)
    lens = rng.integers(0, max_new + 1, size=(nB, N)).astype(np.int32)
    logprobs = (-rng.exponential(1.0, size=(nB, N, max_new))).astype(np.float32)
    for b in range(nB):
        for s in range(N):
            n = lens[b, s]
            if n and rng.random() < 0.7:
                tokens[b, s, n - 1] = eot      # stopped by eot (else: by its budget)
            tokens[b, s, n:] = eot
            logprobs[b, s, n:] = 0.0
    return tokens, lens, logprobs


def test_ranker_against_the_numpy_restatement(pkg):
    rng = np.random.default_rng(3)
    for nB, N, max_new in ((1, 1, 1), (7, 5, 24), (33, 8, 9), (4, 3, 224)):
        tokens, lens, logprobs = _random_candidates(rng, nB, N, max_new, 50)
        for pen in (None, 0.0, 0.3, 1.0):
            best, scores = B.rank_candidates(tokens, lens, logprobs, 50, pen)
            wbest, wscores = rank_np(tokens, lens, logprobs, 50, pen)
            assert np.array_equal(best, wbest), (nB, N, pen)
            # (the sum is the same f64 sum; pow may differ from numpy's ** in the last place)
            assert np.allclose(scores, wscores, rtol=1e-14, atol=0), (nB, N, pen)


def test_ranker_hand_made_cases(pkg):
    E = 9
    inf = float("inf")

    def one(cands, pen):
        """cands: [(tokens, logprobs)] of one row"""
        N, M = len(cands), max(len(t) for t, _ in cands)
        M = max(M, 1)
        tok = np.full((1, N, M), E, np.int32)
        lp = np.zeros((1, N, M), np.float32)
        ln = np.zeros((1, N), np.int32)
        for s, (t, p) in enumerate(cands):
            tok[0, s, :len(t)], lp[0, s, :len(t)], ln[0, s] = t, p, len(t)
        best, sc = B.rank_candidates(tok, ln, lp, E, pen)
        return int(best[0]), sc[0]

    # ties: the first maximal score wins
    assert one([([1, E], [-1, -1]), ([2, E], [-1, -1]), ([3, E], [-0.5, -1.5])], None)[0] == 0
    assert one([([1, E], [-3, -1]), ([2, E], [-1, -1]), ([3, E], [-1, -1])], None)[0] == 1
    # no penalty argument: the sum is divided by the text length -- a longer candidate with the lower sum wins
    a, b = ([1, 2, 3, 4, E], [-1, -1, -1, -1, -0.5]), ([1, E], [-2.0, -0.5])
    best, sc = one([b, a], None)
    assert best == 1 and sc[0] == pytest.approx(-2.5) and sc[1] == pytest.approx(-4.5 / 4)
    # length_penalty 0: the plain sum; 1: (5 + n) / 6; 0.5: its square root
    best, sc = one([b, a], 0.0)
    assert best == 0 and list(sc) == [-2.5, -4.5]
    best, sc = one([b, a], 1.0)
    assert sc[0] == pytest.approx(-2.5 / 1.0) and sc[1] == pytest.approx(-4.5 / 1.5)
    best, sc = one([b, a], 0.5)
    assert sc[1] == pytest.approx(-4.5 / np.sqrt(1.5))
    # n_text == 0 without a penalty: divided by 1 (openai-whisper divides by zero); an empty candidate scores 0
    best, sc = one([([E], [-0.7]), ([1, E], [-0.2, -0.1])], None)
    assert sc[0] == pytest.approx(-0.7) and sc[1] == pytest.approx(-0.3) and best == 1
    best, sc = one([([1, E], [-0.2, -0.1]), ([], [])], None)
    assert sc[1] == 0.0 and best == 1
    # a -inf log-prob is a legal score; every candidate at -inf: candidate 0
    best, sc = one([([1, E], [-inf, -0.1]), ([2, E], [-5, -5])], None)
    assert sc[0] == -inf and best == 1
    best, sc = one([([1, E], [-inf, -0.1]), ([2, E], [-1, -inf]), ([E], [-inf])], 1.0)
    assert np.all(sc == -inf) and best == 0
    # invalid arguments
    tok = np.zeros((1, 2, 3), np.int32)
    ln = np.array([[1, 4]], np.int32)
    with pytest.raises(B.WhisperError):
        B.rank_candidates(tok, ln, np.zeros((1, 2, 3), np.float32), E, None)        # a length beyond max_new
    ln[0, 1] = 2
    for pen in (-0.1, 1.5, float("inf")):
        with pytest.raises(B.WhisperError):
            B.rank_candidates(tok, ln, np.zeros((1, 2, 3), np.float32), E, pen)
    assert b"length_penalty" in B.load_library().wm_last_error()


# ---------------------------------------------------------------- the decode-group cut
def _groups(lib, nB, N, lanes, explicit):
    vp = ctypes.c_void_p
    lib.wmdbg_cand_groups.argtypes = [ctypes.c_int] * 4 + [vp, vp]
    b0 = np.full(nB, -1, np.int32)
    cg = np.full(nB, -1, np.int32)
    G = lib.wmdbg_cand_groups(nB, N, lanes, explicit, b0.ctypes.data_as(vp), cg.ctypes.data_as(vp))
    return G, b0[:max(G, 0)], cg[:max(G, 0)]


def test_candidate_groups_hold_whole_windows_within_the_row_cap(pkg):
    lib = pkg.binding.load_debug_library()
    for N in range(1, 9):
        for nB in list(range(1, 70)) + [128, 200, 257, 1000]:
            for lanes, explicit in ((3, 0), (1, 1), (3, 1), (8, 1)):
                G, b0, cg = _groups(lib, nB, N, lanes, explicit)
                assert 1 <= G <= nB, (nB, N, lanes, explicit, G)
                assert np.all(cg >= 1) and np.all(cg * N <= 128), (nB, N, lanes, cg)
                # every window in exactly one group, in order
                assert b0[0] == 0 and np.array_equal(b0[1:], np.cumsum(cg)[:-1]) and cg.sum() == nB
                assert cg.max() - cg.min() <= 1          # balanced
    # 12 windows x 5 = 60 rows: one group on one lane, wm_group_count's two (>= 32 rows) by default;
    # 40 x 5 = 200 rows span several groups whatever the lanes
    assert _groups(lib, 12, 5, 1, 1)[0] == 1 and _groups(lib, 12, 5, 3, 0)[0] == 2
    G, _, cg = _groups(lib, 40, 5, 3, 0)
    assert G >= 2 and np.all(cg * 5 <= 128)
    G, _, cg = _groups(lib, 40, 5, 1, 1)
    assert G == 2 and list(cg) == [20, 20]
    assert _groups(lib, 16, 8, 3, 0)[0] >= 1 and _groups(lib, 17, 8, 1, 1)[0] == 2
    assert _groups(lib, 4, 9, 3, 0)[0] == -1 and _groups(lib, 0, 2, 3, 0)[0] == -1


# ---------------------------------------------------------------- the candidate word of the Philox counter
_SHIM = r"""
#include "philox.h"
extern "C" {
void shim_bits(uint64_t seed, uint32_t chunk, uint32_t gi, uint32_t n0, int count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = wm_sample_bits(seed, chunk, gi, n0 + (uint32_t)i);
}
void shim_bits_cand(uint64_t seed, uint32_t chunk, uint32_t cand, uint32_t gi, uint32_t n0, int count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = wm_sample_bits_cand(seed, chunk, cand, gi, n0 + (uint32_t)i);
}
}
"""


def sample_bits_cand_np(seed, chunk, cand, gi, n):
    """sample_bits_np with the candidate index as the FOURTH counter word: {n >> 2, gi, chunk, cand}, word n & 3"""
    n = np.asarray(n, dtype=np.uint64)
    ctr = np.stack([n >> np.uint64(2), np.full_like(n, gi), np.full_like(n, chunk), np.full_like(n, cand)], axis=-1)
    out = philox_np(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return np.take_along_axis(out, (n & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def gumbel_cand_np(seed, chunk, cand, gi, n):
    """test_transcribe_options_cpu.gumbel_np restated with the candidate word"""
    from test_transcribe_options_cpu import uniform_np
    return -np.log(-np.log(uniform_np(sample_bits_cand_np(seed, chunk, cand, gi, n))))


def test_candidate_word_of_the_philox_counter(tmp_path):
    src, so = tmp_path / "shim.cpp", tmp_path / "libshim.so"
    src.write_text(_SHIM)
    inc = os.path.join(ROOT, "openai-whisper-coreml_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I", inc, str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.shim_bits.argtypes = [ctypes.c_uint64, u32, u32, u32, ctypes.c_int, vp]
    lib.shim_bits_cand.argtypes = [ctypes.c_uint64, u32, u32, u32, u32, ctypes.c_int, vp]
    n0, cnt = 51000, 866
    ids = np.arange(n0, n0 + cnt)
    seen = []
    for seed, chunk, gi in ((0, 0, 0), (2 ** 40 + 12345, (3 << 16) | 17, 3), (2 ** 64 - 1, 127, 447)):
        plain = np.zeros(cnt, np.uint32)
        lib.shim_bits(seed, chunk, gi, n0, cnt, plain.ctypes.data_as(vp))
        for cand in (0, 1, 4, 7):
            bits = np.zeros(cnt, np.uint32)
            lib.shim_bits_cand(seed, chunk, cand, gi, n0, cnt, bits.ctypes.data_as(vp))
            assert np.array_equal(bits, sample_bits_cand_np(seed, chunk, cand, gi, ids)), (seed, chunk, cand)
            if cand == 0:    # candidate 0 is the stream every other call draws from
                assert np.array_equal(bits, plain) and np.array_equal(bits, sample_bits_np(seed, chunk, gi, ids))
            else:
                assert (bits != plain).mean() > 0.99
            seen.append(bits)
    assert len({b.tobytes() for b in seen}) == len(seen)


# ---------------------------------------------------------------- transcribe_long(best_of=) on a fake context
class FakeCandCtx(FakeCtx):
    """FakeCtx whose transcribe_mel takes best_of: a candidate call answers like the plain one (the selected candidates) and
    says which candidate it kept, (sample id + seed) % best_of."""

    def transcribe_mel(self, *a, best_of=None, length_penalty=None, **kw):
        r = FakeCtx.transcribe_mel(self, *a, **kw)
        self.calls[-1].update(best_of=best_of, length_penalty=length_penalty, seed=kw.get("seed", 0))
        if best_of is not None:
            r.candidate = np.array([(int(s) + int(kw.get("seed", 0))) % best_of for s in kw["sample_ids"]], np.int32)
            for i in range(len(r.candidate)):   # the selected candidate is visible in the tokens that reach the segments
                r.tokens[i, 2] = 3000 + int(r.candidate[i])
        return r


def test_transcribe_long_best_of_on_a_fake_context():
    recs = [np.zeros(16000 * s, np.float32) for s in (25, 12, 38)]
    fb = {(0, 1), (2, 0)}
    plain_ctx = FakeCtx(64, fall_back=fb)
    plain = B.transcribe_long(plain_ctx, recs, seed=40, **_fake_kw())
    ctx = FakeCandCtx(64, fall_back=fb)
    out = B.transcribe_long(ctx, recs, seed=40, best_of=5, length_penalty=0.25, **_fake_kw())
    # the same calls, in the same order, with the same rows, prompts, ids and temperatures
    strip = lambda c: {k: v for k, v in c.items() if k not in ("best_of", "length_penalty", "seed")}
    assert [strip(c) for c in ctx.calls] == plain_ctx.calls
    temps = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    for c in ctx.calls:
        k = temps.index(c["temperature"])
        assert c["seed"] == B.fallback_seed(40, k)                      # the seeds of fallback_decode
        if c["temperature"] == 0.0:
            assert c["best_of"] is None and c["length_penalty"] is None   # the temperature-0 step goes out without candidates
        else:
            assert c["best_of"] == 5 and c["length_penalty"] == 0.25
    assert any(c["temperature"] > 0 for c in ctx.calls)
    # every window record has `candidate`: 0 when its kept step is temperature 0, else what its LAST step kept
    for r, (o, p) in enumerate(zip(out, plain)):
        assert len(o["windows"]) == len(p["windows"])
        for n, (w, pw) in enumerate(zip(o["windows"], p["windows"])):
            assert "candidate" in w and "candidate" not in pw
            assert w["temperatures"] == pw["temperatures"]
            if (r, n) in fb:
                assert w["temperatures"] == [0.0, 0.2, 0.4, 0.6]
                sid = (n << 16) | r
                assert w["candidate"] == (sid + B.fallback_seed(40, 3)) % 5
                assert w["tokens"][2] == 3000 + w["candidate"]          # the selected result reaches the records ...
                assert any(3000 + w["candidate"] in sg["tokens"] for sg in o["segments"] if sg["seek"] == w["seek"])   # ... and the segments
            else:
                assert w["temperatures"] == [0.0] and w["candidate"] == 0 and w["tokens"] == pw["tokens"]
    # best_of=None: the very calls of a context whose transcribe_mel knows nothing of candidates, and no new key
    again_ctx = FakeCtx(64, fall_back=fb)
    again = B.transcribe_long(again_ctx, recs, seed=40, best_of=None, **_fake_kw())
    assert again_ctx.calls == plain_ctx.calls and again == plain


def test_transcribe_with_fallback_best_of_goes_through_logmel_windows():
    calls = []

    class Ctx:
        dims = dict(n_mels=80, n_vocab=1024)

        def transcribe(self, pcm, prompt, max_new, **kw):
            calls.append(("pcm", len(pcm), kw["temperature"], kw["seed"]))
            n = len(pcm)
            return B.TranscribeResult(np.full((n, max_new), EOT, np.int32), np.full(n, 1, np.int32),
                                      np.full((n, max_new), -9.0, np.float32), None, EOT)

        def logmel(self, pcm, n_mels=80):
            return np.zeros((len(pcm), n_mels, 3000), np.float32)

        def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **kw):
            calls.append(("mel", mel.shape, list(mel_base), mel_len, seek, n_frames, kw["temperature"], kw["seed"],
                          kw["best_of"], kw["length_penalty"], kw.get("sample_ids")))
            n = len(mel_base)
            r = B.TranscribeResult(np.full((n, max_new), EOT, np.int32), np.full(n, 1, np.int32),
                                   np.zeros((n, max_new), np.float32), None, EOT)
            r.candidate = np.zeros(n, np.int32)
            return r

    out = B.transcribe_with_fallback(Ctx(), np.zeros((3, 480000), np.float32), [1, 2], 4, EOT, temperatures=(0.0, 0.5),
                                     compression_ratio_threshold=None, seed=7, best_of=5, length_penalty=None)
    assert calls[0] == ("pcm", 3, 0.0, 7)
    assert calls[1] == ("mel", (3, 80, 3000), [0, 240000, 480000], 3000, 0, 3000, 0.5, 8, 5, None, None)
    assert list(out["temperature"]) == [0.5] * 3


# ---------------------------------------------------------------- ISA lint of the candidate cross-attention kernel
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def attn_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("no ROCm toolchain")
    d = tmp_path_factory.mktemp("isa_cand")
    co, elf = str(d / "dec.co"), str(d / "dec.elf")
    src = os.path.join(ROOT, "openai-whisper-coreml_amd", "csrc", "dec_kernels.hip")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "openai-whisper-coreml_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags = [f for f in b.FLAGS if f != "-fPIC"] + b.FILE_FLAGS.get("dec_kernels.hip", [])
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-c", "-x", "hip", src, "-o", co], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + co,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf], check=True, capture_output=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", elf], check=True, capture_output=True,
                         text=True).stdout
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", ln)
        if m:
            cur = m.group(1) if ("dec_xcand_attn_kernel" in m.group(1) or "dec_xrows_attn_kernel" in m.group(1)) else None
            if cur:
                kernels[cur] = []
            continue
        if cur and ln.startswith("\t"):
            ins = ln.split("//")[0].strip()
            if ins and not ins.startswith("s_nop"):
                kernels[cur].append(ins)
    # per kernel: .private_segment_fixed_size of its metadata entry
    private = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and priv:
            private[name.group(1)] = int(priv.group(1))
    return kernels, private


def _compute_prologue(ins):
    """The instructions between the L2 warm-up code and the first K/V load.  Both kernels begin with the warm-up workgroups'
    branch (l2_warm_tile: a loop of plain dwordx4 loads, the first loads in program order), which ends at the first backward
    branch; the K/V rows are the non-temporal 16-byte loads (the queries, also dwordx4, are plain loads in front of them)."""
    warm_end = next(i for i, s in enumerate(ins) if s.startswith("s_cbranch") and int(s.split()[-1]) > 0x7fff)
    first = next(i for i, s in enumerate(ins) if s.startswith("global_load_dwordx4") and s.endswith(" nt"))
    assert warm_end < first and not any(s.startswith("global_load_dwordx4") and s.endswith(" nt") for s in ins[:warm_end])
    return ins[warm_end + 1:first]


def _scalar_memory_waits(block):
    """(scalar loads issued, waits on them) walking the block in program order: an s_waitcnt on lgkmcnt counts as a
    scalar-memory wait when a scalar load has been issued since the last lgkmcnt(0) (scalar loads return out of order, so any
    count waits for them).  The other lgkmcnt waits of the block are the pair loop's: LDS stores of the previous pair's merge,
    nothing outstanding on the way to the FIRST K/V load."""
    loads, waits, pending = [], [], False
    for s in block:
        if s.startswith(("s_load_", "s_buffer_load_")):
            loads.append(s)
            pending = True
        elif s.startswith("s_waitcnt") and "lgkmcnt" in s:
            if pending:
                waits.append(s)
            if "lgkmcnt(0)" in s:
                pending = False
    return loads, waits


def test_candidate_kernel_has_no_scratch_and_no_extra_scalar_wait(attn_isa):
    kernels, private = attn_isa
    cand = sorted(k for k in kernels if "dec_xcand_attn_kernel" in k)
    base = [k for k in kernels if "dec_xrows_attn_kernel" in k]
    assert len(cand) == 8, cand          # best_of 1 .. 8
    assert len(base) >= 1
    for k in cand:
        assert private.get(k) == 0, (k, private.get(k))     # every instantiation: zero private segment
        assert not any(s.startswith(("scratch_", "buffer_store", "buffer_load")) for s in kernels[k]), k
    # the code between the warm-up branch and the first K/V load (the live-list prologue, the window lookup, the queries):
    # no scalar-memory wait beyond what dec_xrows_attn_kernel has there
    allowed = min(len(_scalar_memory_waits(_compute_prologue(kernels[k]))[1]) for k in base)
    assert allowed >= 1          # (its live count; a prologue without any would mean the anchors are wrong)
    for k in cand:
        block = _compute_prologue(kernels[k])
        assert len(block) > 100, (k, len(block))      # the prologue is there: two list loads per lane, ballots, the queries
        loads, waits = _scalar_memory_waits(block)
        assert len(waits) <= allowed, (k, waits, allowed)
        # in fact the live count is the ONE scalar load of the path: everything else arrives as preloaded kernel arguments
        assert len(loads) == 1 and len(waits) == 1, (k, loads, waits)
