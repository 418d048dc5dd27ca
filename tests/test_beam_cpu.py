"""CPU tests of beam-search decoding (include/whisper_mi355x.h wm_transcribe_mel_beam): the selection rule of csrc/beam.h
against the numpy restatement below, the finalize fill-up order, the ranker on the search's sums, the exports, the binding's
argument checks and the transcribe_long / transcribe_with_fallback routing on a fake context.

The decoder, restated (openai-whisper's BeamSearchDecoder; the GPU tests drive BeamWindowNp with the lists the device saw):
  per window N beams with f32 running sums; at generated index gi every live beam j has a list of (token, lp), best first;
  candidates = [(f32(sum_j + lp), j, entry)] for the contributing beams (gi == 0: beam 0 alone), beam-major, stably sorted by
  descending score; walked in order: token == eot -> newly finished (kept while the window has fewer than max_candidates),
  else the next beam until N are taken, where the walk stops; empty slots are dead beams (sum -inf, token pad, lp 0, source
  = the slot).  The window leaves once it has max_candidates finished, or when its budget is used up; finalize appends the live
  beams by descending sum (stable) while there are fewer than N hypotheses."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from beam_step_ref import beam_select_np
from conftest import ROOT
from test_best_of_cpu import rank_np
from test_ragged_prompts_cpu import EOT, FakeCtx, _fake_kw

B = importlib.import_module("openai_whisper_coreml_amd.binding")

MAXN, LIST, HYPS = 8, 9, 16
f32 = np.float32
NINF = f32(-np.inf)


# ---------------------------------------------------------------- the numpy restatement
def fill_order_np(sums):
    live = [j for j in range(len(sums)) if sums[j] != NINF]
    return sorted(live, key=lambda j: -float(sums[j]))


class BeamWindowNp:
    """One window's search, driven step by step with the lists of its beams."""

    def __init__(self, N, max_cand, eot, budget):
        self.N, self.max_cand, self.eot, self.budget = N, max_cand, eot, budget
        self.pad = eot if eot >= 0 else 0
        self.sums = [f32(0)] * N
        self.toks = [[] for _ in range(N)]
        self.lps = [[] for _ in range(N)]
        self.finished = []      # (tokens, lps, sum)
        self.done = False
        self.gi = 0
        self.srcs = []          # per step: the source map

    def step(self, lists):
        assert not self.done
        n_next, src, tok, lp, new, fins = beam_select_np(self.N, 1 if self.gi == 0 else self.N, self.eot, self.pad,
                                                         self.max_cand - len(self.finished), self.sums, lists)
        for j, l, s in fins:
            self.finished.append((self.toks[j] + [self.eot], self.lps[j] + [l], s))
        self.toks = [self.toks[src[k]] + [tok[k]] for k in range(self.N)]
        self.lps = [self.lps[src[k]] + [lp[k]] for k in range(self.N)]
        self.sums = new
        self.srcs.append(list(src))
        self.gi += 1
        self.done = len(self.finished) >= self.max_cand or self.gi >= self.budget

    def hypotheses(self):
        hyps = list(self.finished)
        if len(hyps) < self.N:
            for j in fill_order_np(self.sums):
                if len(hyps) >= self.N:
                    break
                hyps.append((self.toks[j], self.lps[j], self.sums[j]))
        return hyps


def best_np(hyps, eot, length_penalty):
    """rank_np's rule over the search's own sums"""
    best, top = 0, -np.inf
    for h, (toks, _, s) in enumerate(hyps):
        n_text = toks.index(eot) if eot in toks else len(toks)
        if length_penalty is None:
            pen = float(n_text) if n_text > 0 else 1.0
        else:
            pen = ((5.0 + n_text) / 6.0) ** float(f32(length_penalty))
        sc = float(s) / pen
        if sc > top:
            top, best = sc, h
    return best


# ---------------------------------------------------------------- wmdbg_beam_select
def _select(lib, N, n_from, eot, pad, room, sums, lists):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.wmdbg_beam_select.argtypes = [ci, ci, ctypes.c_int32, ctypes.c_int32, ci] + [vp] * 13
    s = np.asarray(sums, f32)
    ln = np.array([len(l) for l in lists], np.int32)
    lt = np.full((N, LIST), -7, np.int32)
    ll = np.full((N, LIST), np.nan, f32)
    for j, l in enumerate(lists):
        for e, (t, p) in enumerate(l):
            lt[j, e], ll[j, e] = t, p
    n_next, n_fin = np.zeros(1, np.int32), np.zeros(1, np.int32)
    src, tok = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    lp, new = np.full(N, np.nan, f32), np.full(N, np.nan, f32)
    fsrc, flp, fsum = np.full(N, -1, np.int32), np.full(N, np.nan, f32), np.full(N, np.nan, f32)
    p = lambda a: a.ctypes.data_as(vp)
    rc = lib.wmdbg_beam_select(N, n_from, eot, pad, room, p(s), p(ln), p(lt), p(ll), p(n_next), p(src), p(tok), p(lp), p(new),
                               p(n_fin), p(fsrc), p(flp), p(fsum))
    assert rc == 0, lib.wm_last_error()
    k = int(n_fin[0])
    return int(n_next[0]), list(src), list(tok), list(lp), list(new), list(zip(fsrc[:k], flp[:k], fsum[:k]))


def _same(got, want):
    gn, gs, gt, gl, gw, gf = got
    wn, ws, wt, wl, ww, wf = want
    assert gn == wn and gs == list(ws) and gt == list(wt)
    assert np.array_equal(np.asarray(gl, f32).view(np.uint32), np.asarray(wl, f32).view(np.uint32))
    assert np.array_equal(np.asarray(gw, f32).view(np.uint32), np.asarray(ww, f32).view(np.uint32))
    assert len(gf) == len(wf)
    for (a, b, c), (x, y, z) in zip(gf, wf):
        assert a == x and f32(b).tobytes() == f32(y).tobytes() and f32(c).tobytes() == f32(z).tobytes()


def _random_lists(rng, N, vocab, eot, p_eot, p_short, quantum):
    lists = []
    for _ in range(N):
        n = N + 1
        if rng.random() < p_short:
            n = int(rng.integers(0, N + 1))
        toks = list(rng.choice(vocab, size=min(n, vocab), replace=False))
        if toks and eot >= 0 and rng.random() < p_eot:
            toks[int(rng.integers(0, len(toks)))] = eot
            toks = list(dict.fromkeys(toks))
        # log-probs on a coarse grid when `quantum` is set: exact score ties across beams and entries
        lp = -rng.exponential(2.0, size=len(toks))
        if quantum:
            lp = np.round(lp / quantum) * quantum
        lp = np.sort(lp.astype(f32))[::-1]
        lists.append([(int(t), f32(v)) for t, v in zip(toks, lp)])
    return lists


def test_select_against_the_numpy_restatement(pkg):
    lib = pkg.binding.load_debug_library()
    rng = np.random.default_rng(11)
    E = 5
    seen = dict(dead=0, ties=0, fins=0, clipped=0, empty=0, first=0)
    for N in range(1, MAXN + 1):
        for max_cand in sorted({max(1, N - 2), N, min(HYPS, N + 3)}):      # below, equal to and above N
            for trial in range(60):
                quantum = 0.5 if trial % 3 == 0 else 0.0
                sums = (-rng.exponential(3.0, size=N)).astype(f32)
                if quantum:
                    sums = (np.round(sums / quantum) * quantum).astype(f32)
                for j in range(N):
                    if rng.random() < 0.15:
                        sums[j] = NINF                                     # a dead beam
                lists = _random_lists(rng, N, 12, E, 0.5, 0.3 if trial % 2 else 0.0, quantum)
                if trial == 7:
                    lists = [[] for _ in range(N)]                         # all lists empty
                n_from = 1 if trial % 5 == 0 else N                       # gi == 0: beam 0 only
                if n_from == 1:
                    sums[:] = 0
                room = int(rng.integers(0, max_cand + 1))
                eot = E if trial % 11 else -1
                want = beam_select_np(N, n_from, eot, E if eot >= 0 else 0, room, list(sums), lists)
                got = _select(lib, N, n_from, eot, E if eot >= 0 else 0, room, sums, lists)
                _same(got, want)
                # the walk's own invariants
                n_next, src, tok, lp, new, fins = want
                assert all(new[k] == NINF and src[k] == k for k in range(n_next, N))
                assert all(float(new[k]) >= float(new[k + 1]) for k in range(n_next - 1))
                seen["dead"] += n_next < N
                seen["fins"] += len(fins) > 0
                seen["first"] += n_from == 1
                seen["empty"] += n_next == 0
                sc = [float(f32(sums[j] + v)) for j in range(n_from) if sums[j] != NINF for _, v in lists[j]]
                seen["ties"] += len(sc) != len(set(sc))
                n_eot = sum(1 for j in range(n_from) if sums[j] != NINF for t, _ in lists[j] if t == eot)
                seen["clipped"] += n_eot > len(fins)
    assert all(v > 10 for v in seen.values()), seen


def test_select_hand_made_cases(pkg):
    lib = pkg.binding.load_debug_library()
    E = 9
    # ties across beams: the lower beam first, then the earlier entry (a stable sort of the beam-major candidate list)
    sums = [f32(-1), f32(-1), f32(-1)]
    lists = [[(1, f32(-1)), (2, f32(-1)), (3, f32(-2))]] * 3
    n, src, tok, lp, new, fins = _select(lib, 3, 3, E, E, 4, sums, lists)
    assert (n, src, tok) == (3, [0, 0, 1], [1, 2, 1]) and fins == []
    # eot in front: finished first, in score order, clipped to the room; the walk stops once N beams are taken
    lists = [[(E, f32(-0.1)), (1, f32(-0.2)), (2, f32(-3))], [(E, f32(-0.15)), (4, f32(-0.3)), (5, f32(-4))],
             [(6, f32(-5)), (E, f32(-6)), (7, f32(-7))]]
    n, src, tok, lp, new, fins = _select(lib, 3, 3, E, E, 1, sums, lists)
    assert (n, src, tok) == (3, [0, 1, 0], [1, 4, 2]) and [f[0] for f in fins] == [0]
    n, src, tok, lp, new, fins = _select(lib, 3, 3, E, E, 5, sums, lists)
    assert [f[0] for f in fins] == [0, 1]          # beam 2's eot lies behind the third taken beam: never seen
    assert fins[1][2] == f32(f32(-1) + f32(-0.15))
    # eot < 0: the id is an ordinary token
    n, src, tok, lp, new, fins = _select(lib, 3, 3, -1, 0, 5, sums, lists)
    assert tok == [E, E, 1] and fins == []
    # short lists: dead beams behind the taken ones; a dead beam brings nothing
    sums = [f32(-2), NINF, f32(-1)]
    lists = [[(1, f32(-1))], [(2, f32(-0.001)), (3, f32(-0.002))], [(E, f32(-0.5))]]
    n, src, tok, lp, new, fins = _select(lib, 3, 3, E, E, 2, sums, lists)
    assert n == 1 and src == [0, 1, 2] and tok == [1, E, E] and new[1] == NINF and new[2] == NINF and lp[1] == 0
    assert [f[0] for f in fins] == [2]
    # the first generated token: beam 0 alone, whatever the others hold
    n, src, tok, lp, new, fins = _select(lib, 3, 1, E, E, 2, [f32(0)] * 3, [[(1, f32(-1)), (2, f32(-2)), (3, f32(-3)), (4, f32(-4))]] * 3)
    assert (n, src, tok) == (3, [0, 0, 0], [1, 2, 3])
    # invalid arguments
    vp = ctypes.c_void_p
    a = np.zeros(16, np.int32).ctypes.data_as(vp)
    assert lib.wmdbg_beam_select(9, 1, E, E, 1, *([a] * 13)) != 0 and b"beam_select" in lib.wm_last_error()
    assert lib.wmdbg_beam_select(3, 4, E, E, 1, *([a] * 13)) != 0


def test_finalize_fill_up_order(pkg):
    lib = pkg.binding.load_debug_library()
    vp = ctypes.c_void_p
    lib.wmdbg_beam_fill_order.argtypes = [ctypes.c_int, vp, vp]
    rng = np.random.default_rng(5)
    for N in range(1, MAXN + 1):
        for _ in range(40):
            sums = (np.round(-rng.exponential(2.0, size=N) * 2) / 2).astype(f32)     # with ties
            sums[rng.random(N) < 0.25] = NINF
            order = np.full(N, -1, np.int32)
            n = lib.wmdbg_beam_fill_order(N, sums.ctypes.data_as(vp), order.ctypes.data_as(vp))
            assert list(order[:n]) == fill_order_np(list(sums)), (N, sums)
    assert lib.wmdbg_beam_fill_order(9, sums.ctypes.data_as(vp), order.ctypes.data_as(vp)) == -1
    # a whole window: 2 finished of 3 wanted at the budget, N = 4 -> two live beams follow, the better sum first
    w = BeamWindowNp(4, 3, 9, budget=2)
    w.step([[(1, f32(-1)), (9, f32(-1.5)), (2, f32(-2)), (3, f32(-3)), (4, f32(-4))]] * 4)
    assert [h[0] for h in w.finished] == [[9]] and not w.done
    w.step([[(9, f32(-0.1)), (5, f32(-0.2))], [(6, f32(-0.1))], [(7, f32(-9))], []])
    assert w.done and [h[0] for h in w.finished] == [[9], [1, 9]]
    hyps = w.hypotheses()
    assert [h[0] for h in hyps] == [[9], [1, 9], [1, 5], [2, 6]]
    assert best_np(hyps, 9, None) == 2 and best_np(hyps, 9, 0.0) == 1   # sums -1.5, -1.1, -1.2, -2.1; n_text 0 counts as 1


def test_ranker_on_sums_follows_rank_np(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_rank_score.restype = ctypes.c_double
    lib.wmdbg_rank_score.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_float]
    rng = np.random.default_rng(2)
    for pen in (None, 0.0, 0.3, 1.0):
        for _ in range(50):
            n = int(rng.integers(0, 30))
            lp = (-rng.exponential(1.0, size=(1, 1, max(n, 1)))).astype(f32)
            tok = np.zeros((1, 1, max(n, 1)), np.int32)
            _, sc = rank_np(tok, np.array([[n]], np.int32), lp, 50, pen)        # no eot among the tokens: n_text = n
            total = float(np.sum(lp[0, 0, :n], dtype=np.float64)) if n else 0.0
            got = lib.wmdbg_rank_score(total, n, float("nan") if pen is None else pen)
            assert got == pytest.approx(sc[0, 0], rel=1e-14, abs=0)
    assert lib.wmdbg_rank_score(-3.0, 0, float("nan")) == -3.0      # n_text == 0 -> 1


# ---------------------------------------------------------------- the ABI
def test_header_declares_and_both_libraries_export_the_call(pkg):
    hdr = open(os.path.join(ROOT, "include", "whisper_mi355x.h")).read()
    assert "WM_API int wm_transcribe_mel_beam(" in hdr
    assert "#define WM_MAX_BEAM 8" in hdr and "#define WM_MAX_BEAM_HYPS 16" in hdr
    assert B.MAX_BEAM == 8 and B.MAX_BEAM_HYPS == 16
    for lib in (pkg.binding.load_library(), pkg.binding.load_debug_library()):
        assert hasattr(lib, "wm_transcribe_mel_beam")
    dbg = pkg.binding.load_debug_library()
    for name in ("wmdbg_beam_select", "wmdbg_beam_fill_order", "wmdbg_beam_trace", "wmdbg_beam_topk", "wmdbg_beam_reorder",
                 "wmdbg_beam_step", "wmdbg_beam_step_layout"):
        assert hasattr(dbg, name), name
        assert not hasattr(pkg.binding.load_library(), name), name


def test_argument_checks(pkg):
    # the binding's own rule
    assert B.beam_max_candidates(5, None) == 5 and B.beam_max_candidates(5, 2.0) == 10 and B.beam_max_candidates(None) is None
    assert B.beam_max_candidates(5, 0.5) == round(2.5) == 2 and B.beam_max_candidates(3, 0.5) == round(1.5) == 2   # Python's round
    for bs, pat in ((0, None), (9, None), (2.5, None), (5, 0.0), (5, -1.0), (8, 2.5), (1, 0.4), (None, 1.0)):
        with pytest.raises(ValueError):
            B.beam_max_candidates(bs, pat)
    # the C entry point rejects its own arguments before it looks at the context
    lib = pkg.binding.load_library()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    opts = B.wm_decode_opts(0.0, 0, -1, 0)

    def call(beam, cand, pen=float("nan"), n_hyp=p, sums=p, B_=1, max_new=4, stride=3):
        return lib.wm_transcribe_mel_beam(None, p, p, p, p, p, B_, p, stride, None, 1, beam, cand, pen, max_new, 7, ctypes.byref(opts),
                                          p, p, n_hyp, sums, None, None, None, 0)
    for args, word in (((0, 1), b"beam_size"), ((9, 1), b"beam_size"), ((5, 0), b"max_candidates"), ((5, 17), b"max_candidates"),
                       ((5, 5, 1.5), b"length_penalty"), ((5, 5, -0.5), b"length_penalty")):
        assert call(*args) != 0
        assert word in lib.wm_last_error(), (args, lib.wm_last_error())
    assert call(5, 5, n_hyp=None) != 0 and b"n_hyp_out" in lib.wm_last_error()
    assert call(5, 5, sums=None) != 0
    assert call(5, 5, B_=0) != 0 and call(5, 5, max_new=0) != 0 and call(5, 5, stride=0) != 0
    assert call(5, 5) != 0          # valid beam arguments: now the null context is what is wrong


# ---------------------------------------------------------------- routing on a fake context
class FakeBeamCtx(FakeCtx):
    """FakeCtx whose transcribe_mel takes beam_size / patience (and best_of): a beam call answers like the plain one and says
    which hypothesis it kept, sample id % beam_size."""

    def transcribe_mel(self, *a, best_of=None, length_penalty=None, beam_size=None, patience=None, **kw):
        r = FakeCtx.transcribe_mel(self, *a, **kw)
        self.calls[-1].update(best_of=best_of, length_penalty=length_penalty, beam_size=beam_size, patience=patience)
        if best_of is not None:
            r.candidate = np.array([int(s) % best_of for s in kw["sample_ids"]], np.int32)
        if beam_size is not None:
            assert kw.get("temperature", 0.0) == 0.0
            r.hypothesis = np.array([int(s) % beam_size for s in kw["sample_ids"]], np.int32)
            for i in range(len(r.hypothesis)):
                r.tokens[i, 2] = 3000 + int(r.hypothesis[i])
        return r


def test_transcribe_long_routes_the_temperature_0_step_to_the_beam_call():
    recs = [np.zeros(16000 * s, np.float32) for s in (25, 12, 38)]
    fb = {(0, 1), (2, 0)}
    plain_ctx = FakeCtx(64, fall_back=fb)
    plain = B.transcribe_long(plain_ctx, recs, seed=40, **_fake_kw())
    ctx = FakeBeamCtx(64, fall_back=fb)
    out = B.transcribe_long(ctx, recs, seed=40, beam_size=5, patience=2.0, best_of=3, length_penalty=0.25, **_fake_kw())
    strip = lambda c: {k: v for k, v in c.items() if k not in ("best_of", "length_penalty", "beam_size", "patience")}
    assert [strip(c) for c in ctx.calls] == plain_ctx.calls        # the same calls, rows, prompts, ids and temperatures
    assert any(c["temperature"] > 0 for c in ctx.calls)
    for c in ctx.calls:
        if c["temperature"] == 0.0:    # the temperature-0 step carries beam_size, and no best_of
            assert (c["beam_size"], c["patience"], c["best_of"], c["length_penalty"]) == (5, 2.0, None, 0.25)
        else:                          # later steps carry best_of only
            assert (c["beam_size"], c["patience"], c["best_of"], c["length_penalty"]) == (None, None, 3, 0.25)
    for r, (o, p) in enumerate(zip(out, plain)):
        for n, (w, pw) in enumerate(zip(o["windows"], p["windows"])):
            assert "hypothesis" in w and "hypothesis" not in pw
            sid = (n << 16) | r
            if (r, n) in fb:
                assert w["hypothesis"] == 0 and w["candidate"] == sid % 3       # a later step replaced the beam result
            else:
                assert w["hypothesis"] == sid % 5 and w["candidate"] == 0
                assert w["tokens"][2] == 3000 + w["hypothesis"]                 # the kept hypothesis reaches the records ...
                assert any(3000 + w["hypothesis"] in sg["tokens"] for sg in o["segments"] if sg["seek"] == w["seek"])   # ... and the segments
    # beam_size None: the very calls of a context that knows nothing of beams, and no new key
    again_ctx = FakeCtx(64, fall_back=fb)
    again = B.transcribe_long(again_ctx, recs, seed=40, beam_size=None, **_fake_kw())
    assert again_ctx.calls == plain_ctx.calls and again == plain
    with pytest.raises(ValueError):
        B.transcribe_long(FakeBeamCtx(64), recs, patience=1.0, **_fake_kw())
    with pytest.raises(ValueError):
        B.transcribe_long(FakeBeamCtx(64), recs, beam_size=9, **_fake_kw())


def test_transcribe_with_fallback_routes_the_temperature_0_step_to_the_beam_call():
    calls = []

    class Ctx:
        dims = dict(n_mels=80, n_vocab=1024)

        def transcribe(self, pcm, prompt, max_new, **kw):
            calls.append(("pcm", len(pcm), kw["temperature"], kw["seed"]))
            n = len(pcm)
            return B.TranscribeResult(np.full((n, max_new), EOT, np.int32), np.full(n, 1, np.int32),
                                      np.zeros((n, max_new), f32), None, EOT)

        def logmel(self, pcm, n_mels=80):
            return np.zeros((len(pcm), n_mels, 3000), f32)

        def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, **kw):
            calls.append(("mel", mel.shape, kw["temperature"], kw["seed"], kw.get("beam_size"), kw.get("patience"),
                          kw.get("best_of"), kw.get("length_penalty")))
            n = len(mel_base)
            r = B.TranscribeResult(np.full((n, max_new), EOT, np.int32), np.full(n, 1, np.int32),
                                   np.full((n, max_new), -9.0, f32), None, EOT)   # low log-probs: every row falls back
            r.hypothesis = np.zeros(n, np.int32)
            return r

    out = B.transcribe_with_fallback(Ctx(), np.zeros((3, 480000), f32), [1, 2], 4, EOT, temperatures=(0.0, 0.5),
                                     compression_ratio_threshold=None, seed=7, beam_size=4, patience=1.5, length_penalty=0.5)
    assert calls[0] == ("mel", (3, 80, 3000), 0.0, 7, 4, 1.5, None, 0.5)      # the beam call, over the chunks' log-mel windows
    assert calls[1] == ("pcm", 3, 0.5, 8)                                      # above temperature 0: unchanged
    assert list(out["temperature"]) == [0.5] * 3
    with pytest.raises(ValueError):
        B.transcribe_with_fallback(Ctx(), np.zeros((1, 480000), f32), [1, 2], 4, EOT, patience=2.0)
