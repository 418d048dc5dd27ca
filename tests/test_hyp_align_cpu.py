"""CPU tests of the host side of decode-pass word timestamps for best-of and beam-search hypotheses: wm_beam_ancestry (through
wmdbg_beam_ancestry) on random multi-step searches driven by wmdbg_beam_select, against a numpy restatement of the walk and
against histories carried by copy; transcribe_long's word_timestamps="decode_best" on the recording fake -- its call sequence,
words and ValueErrors --; and the transcribe plan's row bound with five rows per window."""
import ctypes
import importlib
import types

import numpy as np
import pytest

from test_decode_align_cpu import AlignedCtx, _grid, _plans, _run, _timing, dbg, vocab   # noqa: F401  (fixtures)
from test_longform_calls_cpu import LANGS, SCRIPT, STD
from test_longform_words_cpu import EOT, NO_TS

B = importlib.import_module("openai_whisper_coreml_amd.binding")
IP = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
MAX_BEAM, MAX_HYPS, LIST = 8, 16, 9


def _ip(a):
    return a.ctypes.data_as(IP)


def _fp(a):
    return a.ctypes.data_as(FP)


@pytest.fixture(scope="module")
def lib(pkg):
    d = pkg.binding.load_debug_library()
    d.wmdbg_beam_select.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, FP, IP, IP, FP, IP, IP,
                                    IP, FP, FP, IP, IP, FP, FP]
    d.wmdbg_beam_select.restype = ctypes.c_int
    d.wmdbg_beam_ancestry.argtypes = [ctypes.c_int, ctypes.c_int, IP, ctypes.c_int, IP, IP, ctypes.c_int, FP, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, IP]
    d.wmdbg_beam_ancestry.restype = ctypes.c_int
    return d


# ---------------------------------------------------------------- the ancestry walk
def _search(lib, rng, N, max_cand, max_new, budget, eot, p_eot, p_short):
    """One window's search as the select kernel runs it, histories carried by COPY (openai-whisper's way).  Returns the state
    wm_beam_ancestry reads, the hypotheses in output order (tokens, finished?) and fed[(slot, gi)]: the history the row in
    `slot` is fed at the step behind close gi."""
    pad = eot if eot >= 0 else 0
    s = np.zeros(N, dtype=np.float32)
    hist = [[] for _ in range(N)]
    anc = np.tile(np.arange(N, dtype=np.int32), (max_new, 1))
    fin_src, fin_len, fin_tok, fed = [], [], [], {}
    wsteps = 0
    for gi in range(max_new):
        ln = np.zeros(N, dtype=np.int32)
        lt = np.zeros((N, LIST), dtype=np.int32)
        ll = np.zeros((N, LIST), dtype=np.float32)
        for j in range(N):
            if s[j] == -np.inf:
                continue
            ln[j] = rng.integers(0, N + 2) if rng.random() < p_short else N + 1
            toks = rng.choice(np.arange(100, 100 + 4 * LIST), size=LIST, replace=False)   # distinct within a list
            if eot >= 0 and rng.random() < p_eot:
                toks[rng.integers(0, 3)] = eot
            lt[j] = toks
            ll[j] = -np.sort(rng.random(LIST).astype(np.float32) * 3)
        out = [np.zeros(1, np.int32), np.zeros(MAX_BEAM, np.int32), np.zeros(MAX_BEAM, np.int32), np.zeros(MAX_BEAM, np.float32),
               np.zeros(MAX_BEAM, np.float32), np.zeros(1, np.int32), np.zeros(MAX_BEAM, np.int32), np.zeros(MAX_BEAM, np.float32),
               np.zeros(MAX_BEAM, np.float32)]
        n_next, src, tok, lp, new_sum, n_fin, fsrc, flp, fsum = out
        assert lib.wmdbg_beam_select(N, 1 if gi == 0 else N, eot, pad, max_cand - len(fin_src), _fp(s), _ip(ln), _ip(lt), _fp(ll),
                                     _ip(n_next), _ip(src), _ip(tok), _fp(lp), _fp(new_sum), _ip(n_fin), _ip(fsrc), _fp(flp),
                                     _fp(fsum)) == 0
        for f in range(int(n_fin[0])):
            fin_src.append(int(fsrc[f]))
            fin_len.append(gi + 1)
            fin_tok.append(list(hist[fsrc[f]]) + [eot])
        hist = [list(hist[src[k]]) + [int(tok[k])] for k in range(N)]     # by copy
        s = new_sum[:N].copy()
        anc[gi] = src[:N]
        for k in range(N):
            fed[(k, gi)] = tuple(hist[k])
        wsteps = gi + 1
        if len(fin_src) >= max_cand or gi + 1 >= budget:
            break
    live = [j for j in sorted(range(N), key=lambda j: (-s[j], j)) if s[j] != -np.inf]
    hyps = [(t, True, None) for t in fin_tok] + [(hist[j], False, j) for j in live][:max(N - len(fin_tok), 0)]
    state = dict(anc=np.ascontiguousarray(anc), fin_n=len(fin_src), fin_src=np.array(fin_src + [0], dtype=np.int32),
                 fin_len=np.array(fin_len + [0], dtype=np.int32), wsteps=wsteps, sum=s)
    return state, hyps, fed


def _walk(anc, k, gi, S, Tq):
    """the numpy restatement: slot_after[gi] = k, slot_after[g - 1] = anc[g][slot_after[g]]; the prompt rows take the end"""
    slot = np.full(Tq, k, dtype=np.int32)
    for g in range(gi, -1, -1):
        if S + 1 + g < Tq:
            slot[S + 1 + g] = k
        k = int(anc[g][k])
    slot[:S + 1] = k
    return slot


def test_the_walk_returns_every_hypothesis_own_prefix(lib):
    rng = np.random.default_rng(2117)
    seen = dict(finished=0, live=0, len1_live=0, first_token_finish=0, dead=0, early=0, moved=0, searches=0)
    cases = [(N, mc, eot) for N in range(1, 9) for mc in sorted({max(1, N - 1), N, min(N + 3, MAX_HYPS)}) for eot in (EOT, -1)]
    for N, max_cand, eot in cases:
        for rep in range(6):
            max_new = int(rng.integers(1, 14))
            budget = 1 if rep == 0 else int(rng.integers(1, max_new + 1)) if rep < 3 else max_new
            p_eot = 0.9 if rep == 1 else 0.25
            state, hyps, fed = _search(lib, rng, N, max_cand, max_new, budget, eot, p_eot, p_short=0.3 if rep % 2 else 0.0)
            S = int(rng.integers(0, 4))
            Tq = S + max_new
            seen["searches"] += 1
            seen["dead"] += int((state["sum"] == -np.inf).any())
            seen["early"] += int(state["wsteps"] < max_new)
            for h, (toks, finished, beam) in enumerate(hyps):
                slot = np.full(Tq, -7, dtype=np.int32)
                got = lib.wmdbg_beam_ancestry(N, max_new, _ip(state["anc"]), state["fin_n"], _ip(state["fin_src"]),
                                              _ip(state["fin_len"]), state["wsteps"], _fp(state["sum"]), h, S, Tq, _ip(slot))
                assert got == len(toks), (N, max_cand, h)
                start, gi = (state["fin_src"][h], len(toks) - 2) if finished else (beam, len(toks) - 1)
                assert np.array_equal(slot, _walk(state["anc"], int(start), gi, S, Tq)), (N, max_cand, h)
                assert ((slot >= 0) & (slot < N)).all()
                # capture row S + 1 + gi was fed the hypothesis' own first gi + 1 tokens, by whoever held them then
                for g in range(len(toks) - 1):
                    assert fed[(int(slot[S + 1 + g]), g)] == tuple(toks[:g + 1]), (N, max_cand, h, g)
                assert (slot[:S + 1] == 0).all()     # the first close continues beam 0 alone
                seen["finished" if finished else "live"] += 1
                seen["len1_live"] += int(not finished and len(toks) == 1)
                seen["first_token_finish"] += int(finished and len(toks) == 1)
                seen["moved"] += int(len(set(slot[S + 1:S + len(toks)].tolist())) > 1)
            slot = np.zeros(Tq, dtype=np.int32)
            assert lib.wmdbg_beam_ancestry(N, max_new, _ip(state["anc"]), state["fin_n"], _ip(state["fin_src"]), _ip(state["fin_len"]),
                                           state["wsteps"], _fp(state["sum"]), len(hyps), S, Tq, _ip(slot)) == -1
    assert all(v > 0 for v in seen.values()), seen
    # bad arguments
    a = np.zeros((2, 2), dtype=np.int32)
    z, s2, slot = np.zeros(1, np.int32), np.zeros(2, np.float32), np.zeros(4, np.int32)
    assert lib.wmdbg_beam_ancestry(9, 2, _ip(a), 0, _ip(z), _ip(z), 1, _fp(s2), 0, 0, 4, _ip(slot)) == -2
    a[1, 0] = 2
    assert lib.wmdbg_beam_ancestry(2, 2, _ip(a), 0, _ip(z), _ip(z), 1, _fp(s2), 0, 0, 4, _ip(slot)) == -2


# ---------------------------------------------------------------- transcribe_long(word_timestamps="decode_best") on the fake
class HypCtx(AlignedCtx):
    """AlignedCtx with the four aligned best-of / beam entries.  The beam entries take no sample ids, so a window is found by
    its recording (the log-mel offset) and its ordinal among the recording's windows (seeks in order of first appearance) --
    checked against the sample ids wherever a call carries them."""

    def __init__(self, *a, **kw):
        AlignedCtx.__init__(self, *a, **kw)
        self.offs, self.ordinal = None, {}

    def logmel_long(self, *a, **kw):
        r = AlignedCtx.logmel_long(self, *a, **kw)
        self.offs = [int(x) for x in r[1]]
        return r

    def encode_windows(self, *a, **kw):
        s = AlignedCtx.encode_windows(self, *a, **kw)
        s.where = list(zip(a[1], a[3]))
        return s

    def _sids(self, where, given=None):
        out = []
        for base, seek in where:
            rec = self.offs.index(int(base))
            seeks = self.ordinal.setdefault(rec, [])
            if int(seek) not in seeks:
                seeks.append(int(seek))
            out.append((seeks.index(int(seek)) << 16) | rec)
        assert given is None or out == [int(s) for s in given]
        return out

    def _hyp(self, ids, max_new, kw, key, n):
        r = self._decode(ids, max_new, dict(kw, temperature=kw.get("temperature", 0.0), **{key: n}))
        start = self._aligned(r, ids, max_new).start_frames
        return types.SimpleNamespace(selected=r, best=r.hypothesis if key == "beam_size" else r.candidate, start_frames=start)

    def transcribe_mel_beam_aligned(self, *a, **kw):
        self._log("transcribe_mel_beam_aligned", a, kw)
        return self._hyp(self._sids(zip(a[1], a[3])), a[6], kw, "beam_size", a[7])

    def transcribe_windows_beam_aligned(self, *a, **kw):
        self._log("transcribe_windows_beam_aligned", a, kw)
        return self._hyp(self._sids([a[0].where[int(r)] for r in a[1]]), a[3], kw, "beam_size", a[4])

    def transcribe_mel_best_of_aligned(self, *a, **kw):
        self._log("transcribe_mel_best_of_aligned", a, kw)
        return self._hyp(self._sids(zip(a[1], a[3]), kw["sample_ids"]), a[6], kw, "best_of", a[7])

    def transcribe_windows_best_of_aligned(self, *a, **kw):
        self._log("transcribe_windows_best_of_aligned", a, kw)
        return self._hyp(self._sids([a[0].where[int(r)] for r in a[1]], kw["sample_ids"]), a[3], kw, "best_of", a[4])

    def transcribe_mel_aligned(self, *a, **kw):
        self._sids(zip(a[1], a[3]), kw["sample_ids"])
        return AlignedCtx.transcribe_mel_aligned(self, *a, **kw)

    def transcribe_windows_aligned(self, *a, **kw):
        self._sids([a[0].where[int(r)] for r in a[1]], kw["sample_ids"])
        return AlignedCtx.transcribe_windows_aligned(self, *a, **kw)


def _as_aligned(call):
    """the call "decode_best" makes where word_timestamps=True makes the plain decode call `call`"""
    name, args, kw = call
    if name not in ("transcribe_mel", "transcribe_windows"):
        return call
    d = dict((k, v) for k, v in kw)
    if "beam_size" in d:
        n = d.pop("beam_size")
        for k in ("temperature", "seed", "sample_ids"):
            d.pop(k)
        return [name + "_beam_aligned", args + [n], sorted([k, v] for k, v in d.items())]
    if "best_of" in d:
        n = d.pop("best_of")
        return [name + "_best_of_aligned", args + [n], sorted([k, v] for k, v in d.items())]
    return [name + "_aligned", args, kw]


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("mode", [dict(best_of=3, length_penalty=0.5), dict(beam_size=2, patience=1.5),
                                  dict(beam_size=3, best_of=2, length_penalty=1.0), dict()])
def test_decode_best_call_sequence_and_words_on_the_fake(vocab, reuse, mode):
    """Every decode call of the run is the aligned entry that matches the fallback step -- beam search at temperature 0,
    best-of above it, the plain aligned entry otherwise -- with the arguments the plain entry gets under word_timestamps=True
    (a beam entry: less temperature, seed and sample ids), no align* call is made, and the words are those of
    word_timestamps=True on the fake's scripted frames."""
    kw = dict(STD, vocab=vocab, language=LANGS, reuse_encoder=reuse, **mode)
    a, t = HypCtx(SCRIPT), HypCtx(SCRIPT)
    got = _run(a, word_timestamps="decode_best", **kw)
    want = _run(t, word_timestamps=True, no_timestamps=NO_TS, **kw)
    names = [c[0] for c in a.calls]
    assert not [n for n in names if n.startswith("align")]
    assert "transcribe_mel" not in names and "transcribe_windows" not in names
    kind = "windows" if reuse else "mel"
    assert ("transcribe_%s_beam_aligned" % kind in names) == ("beam_size" in mode)
    assert ("transcribe_%s_best_of_aligned" % kind in names) == ("best_of" in mode)
    # (the plain aligned entry: temperature 0 without beam_size, the steps above it without best_of)
    assert ("transcribe_%s_aligned" % kind in names) == (not ("beam_size" in mode and "best_of" in mode))
    rest = [c for c in t.calls if not c[0].startswith("align")]
    assert [_as_aligned(c) for c in rest] == a.calls
    assert _timing(got) == _timing(want)
    assert [o["seeks"] for o in got] == [o["seeks"] for o in want]
    assert [o["windows"] for o in got] == [o["windows"] for o in want]     # (candidate / hypothesis of the kept step included)
    pg = [w["probability"] for o in got for s in o["segments"] for w in s.get("words", [])]
    pw = [w["probability"] for o in want for s in o["segments"] for w in s.get("words", [])]
    assert len(pg) > 0 and np.allclose(pg, pw, rtol=1e-6, atol=0)
    windows = [w for o in got for w in o["windows"]]
    assert any(len(w["temperatures"]) > 1 for w in windows) and any(w["skipped"] for w in windows)
    if not mode:     # neither: "decode" exactly
        d = HypCtx(SCRIPT)
        assert _timing(_run(d, word_timestamps="decode", **kw)) == _timing(got) and d.calls == a.calls


def test_decode_best_value_errors_come_before_any_library_call(vocab):
    for kw in (dict(word_timestamps="decode_best"),                                    # no vocab
               dict(word_timestamps="decode_bes", vocab=vocab),                        # no such mode
               dict(word_timestamps="decode_best", vocab=vocab, patience=2.0),         # patience without beam_size
               dict(word_timestamps="decode_best", vocab=vocab, beam_size=9),
               dict(word_timestamps="decode", vocab=vocab, beam_size=2),               # as before
               dict(word_timestamps="decode", vocab=vocab, best_of=2)):
        ctx = HypCtx(SCRIPT)
        with pytest.raises(ValueError):
            _run(ctx, **dict(STD, **kw))
        assert ctx.calls == [], kw


# ---------------------------------------------------------------- the plan's bound with five rows per window
@pytest.mark.parametrize("bound", [3, 5, 12, 48, 97, 128])
def test_with_five_rows_per_window_a_group_keeps_whole_windows_within_the_bound(dbg, bound):
    N = 5
    w_max = max(1, bound // N)     # (a bound below one window still gives every group one)
    for a, (L, parts, G, n_lanes, kind) in _grid((N,), ((0, 2), (0,), (0,))):
        out, cut = _plans(dbg, a, bound)
        Bn, Gb, start = a[:, 0].astype(np.int64), out[:, 2].astype(np.int64), out[:, 5].astype(np.int64)
        assert (Gb >= -(-Bn // w_max)).all() and (Gb <= Bn).all()
        assert (out[:, 1] == 0).all()     # no sub-chip parts for candidate groups
        for i in np.random.default_rng(bound).choice(len(a), size=300, replace=False):
            g = int(Gb[i])
            b0, cg = cut[start[i]:start[i] + g], cut[start[i] + g:start[i] + 2 * g]
            assert cg.sum() == Bn[i] and cg.min() >= 1 and cg.max() - cg.min() <= 1
            assert cg.max() <= min(w_max, 128 // N) and (cg.max() * N <= bound or cg.max() == 1), (a[i, :10], bound)
            assert b0[0] == 0 and np.array_equal(b0[1:], np.cumsum(cg)[:-1])
