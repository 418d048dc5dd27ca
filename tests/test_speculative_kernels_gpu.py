"""Kernel-level GPU tests of the bookkeeping kernels of a speculative round (csrc/spec.hip): spec_adopt_kernel,
spec_stage_kernel and spec_commit_kernel, each driven alone on caller-given state through wmdbg_spec_kernel
(include/whisper_mi355x_debug.h; which = 0 / 1 / 2), the rules of the target and of the draft on or off independently.  The right
answer is exact: every comparison is array_equal on integers or raw float bits against the plain-Python restatement
tests/spec_ref.py (adopt_ref, stage_ref, commit_ref, ts_advance), which tests/test_speculative_plan_cpu.py holds to the oracle's
ApplyTimestampRules and to hand-worked cases first.  Every buffer goes in pre-filled with a sentinel (ints SENT, floats the NaN
bits WMDBG_SENTINEL_F32, the token buffers a different negative value per cell) and comes back whole, per-window arrays with
rows behind the group's: "nothing else was written" is part of every comparison.

Vocabularies: tiny (1024, timestamps from 900, eot 890, max_initial 20) and production (51865, 50364, 50257).  n_ctx = 64.
  test_adopt                           spec_adopt_kernel   G 1 / 5 / 64 / 65 / 128 x the four (target, draft) rule settings
  test_stage                           spec_stage_kernel   (G, w) of SHAPES, rules on / off, (a) the draft's tokens, (b) a script
                                                           that ends inside the panel, (c) ids outside the vocabulary, (d) the
                                                           end of the context
  test_commit_against_the_restatement  spec_commit_kernel  (G, w) of SHAPES x 40 seeded cases, the draw's coverage asserted
  test_rounds_chained                  all three           adopt, then 8 rounds of stage -> commit over 5 windows x 4 rows
SHAPES = (1, 1), (1, 8), (5, 3), (16, 8), (42, 3), (64, 2), (128, 1): G x w <= 128 up to the bound, one and many windows.

MEASURED on the MI355X (wall per test, the hook's uploads and downloads included; every case passes, no kernel changed):
  test_adopt 0.02 s per vocabulary (20 launches); test_stage 0.01 - 0.03 s per shape (12 launches);
  test_commit_against_the_restatement 0.03 - 0.12 s per shape (40 launches; the restatement is most of it: 0.11 s at 128 x 1,
  0.12 s at 1 x 8 in one run, 0.03 s in another); test_rounds_chained 0.01 s (17 launches); the file 1.4 s.
"""
import ctypes
import functools

import numpy as np
import pytest

import spec_ref as S

pytestmark = pytest.mark.gpu

vp, i32 = ctypes.c_void_p, ctypes.c_int32
SENT = -7777                                   # ints nothing may write
SENT_F32 = 0x7fc0dead                          # WMDBG_SENTINEL_F32
N_CTX, P0 = 64, 3                              # the context, the prompt length
VOCABS = {"tiny": (900, 890, 1024, 20), "production": (50364, 50257, 51865, 50)}     # ts_begin, eot, n_vocab, max_initial
SHAPES = [(1, 1), (1, 8), (5, 3), (16, 8), (42, 3), (64, 2), (128, 1)]
STATE4 = ("tts_hist", "dts_hist", "dts_rng", "chist", "crng", "dchist", "dcrng", "stats")      # [cap][4]
INTS = ("tseq", "dseq", "pos2", "tts_rng", "wtok", "acc", "done", "round", "n_live") + STATE4
FLOATS = ("wlp", "logprob")


class Spec(ctypes.Structure):
    """struct wmdbg_spec"""
    _fields_ = [(n, i32) for n in ("which", "G", "w", "cap", "n_prompt", "n_ctx", "max_new", "n_vocab", "tts_on", "dts_on")] + \
               [("tts_par", i32 * 4), ("dts_par", i32 * 4), ("eot", i32), ("pad_tok", i32)] + \
               [(n, vp) for n in ("script", "budget", "tseq", "dseq", "pos2", "tts_hist", "tts_rng", "dts_hist", "dts_rng", "chist", "crng",
                                  "dchist", "dcrng", "wtok", "wlp", "acc", "done", "stats", "round", "n_live", "logprob")]


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_spec_kernel.argtypes = [vp, ctypes.POINTER(Spec)]
    lay = (i32 * 4)()      # the ctypes restatement above against the header's struct
    assert c.lib.wmdbg_spec_layout(lay) == 0
    assert list(lay) == [ctypes.sizeof(Spec), Spec.tts_par.offset, Spec.script.offset, Spec.logprob.offset], list(lay)
    yield c
    c.close()


def fresh(G, w, max_new, pos, cap=None):
    """a state nobody has written: every array at its sentinel, the positions at pos"""
    cap = G + 3 if cap is None else cap
    st = {k: np.full((cap, 4), SENT, np.int32) for k in STATE4}
    st.update(tts_rng=np.full((cap * w, 4), SENT, np.int32), wtok=np.full(cap * w, SENT, np.int32), acc=np.full(cap, SENT, np.int32),
              done=np.full(cap, SENT, np.int32), round=np.full(2, SENT, np.int32), n_live=np.full(1, SENT, np.int32),
              pos2=np.array([pos, pos], np.int32), script=None, budget=None,
              tseq=-(1000 + np.arange(N_CTX * G, dtype=np.int32)).reshape(N_CTX, G),
              dseq=-(900000 + np.arange(N_CTX * G, dtype=np.int32)).reshape(N_CTX, G),
              wlp=np.full(cap * w, SENT_F32, np.uint32).view(np.float32), logprob=np.full((max_new, G), SENT_F32, np.uint32).view(np.float32))
    return st


def as_int(a):
    return a.view(np.uint32).astype(np.int64) if a.dtype == np.float32 else a.astype(np.int64)


def lists(st):
    """the state as spec_ref takes it: nested lists, floats as their bit patterns"""
    out = {k: (None if v is None else as_int(v).tolist()) for k, v in st.items()}
    out["pos"] = int(st["pos2"][0])
    return out


def run(dbg, which, st, G, w, max_new, vocab, tts_on, dts_on, eot=-1, pad_tok=0, n_prompt=P0, n_vocab=None):
    """one wmdbg_spec_kernel call on copies of st's arrays -> the state behind it"""
    out = {k: (None if v is None else np.ascontiguousarray(v).copy()) for k, v in st.items()}
    io = Spec()
    io.which, io.G, io.w, io.cap = which, G, w, out["acc"].shape[0]
    io.n_prompt, io.n_ctx, io.max_new, io.n_vocab = n_prompt, N_CTX, max_new, vocab[2] if n_vocab is None else n_vocab
    io.tts_on, io.dts_on, io.eot, io.pad_tok = int(tts_on), int(dts_on), eot, pad_tok
    io.tts_par[:] = vocab
    io.dts_par[:] = vocab
    for k, v in out.items():
        setattr(io, k, None if v is None else v.ctypes.data_as(vp))
    assert dbg.lib.wmdbg_spec_kernel(dbg.handle, ctypes.byref(io)) == 0, dbg.lib.wm_last_error()
    return out


def same(out, st, ref, what):
    """every array of the state behind the launch: what the restatement wrote where it wrote, the input everywhere else"""
    want = dict(lists(st))
    want.update({k: v for k, v in ref.items() if k in want})
    if "tpos" in ref:
        want["pos2"] = [ref["tpos"], ref["dpos"]]
    if "n_live" in ref:
        want["n_live"] = [ref["n_live"]]
    for k in INTS + FLOATS:
        assert np.array_equal(as_int(out[k]), np.array(want[k], dtype=np.int64).reshape(out[k].shape)), (what, k)
    for k in ("script", "budget"):
        assert st[k] is None or np.array_equal(out[k], st[k]), (what, k)


def rules_of(vocab, on):
    return vocab if on else None


@functools.lru_cache(maxsize=None)
def histories(vocab):
    """the committed states the windows start from: the CPU test's set of histories in this vocabulary (the last timestamp id is
    behind max_initial in both, so fewer open a transcript than there)"""
    tsb, eot, V, _ = vocab
    hs, left_out = S.rule_histories((5, 17, eot, tsb, tsb + 1, tsb + 7, V - 1), vocab)
    assert (len(hs), left_out) == (946, 19608 - 946)
    return hs


# ---------------------------------------------------------------- adopt
@pytest.mark.parametrize("vname", sorted(VOCABS))
def test_adopt(dbg, vname):
    vocab = VOCABS[vname]
    tsb, eot, V, maxi = vocab
    for G in (1, 5, 64, 65, 128):
        for tts_on, dts_on in ((0, 0), (1, 1), (1, 0), (0, 1)):
            st = fresh(G, 1, 8, P0)
            # the first token of window c: text, eot, a timestamp <= max_initial, the last timestamp id
            first = [(7 + c, eot, tsb + c % (maxi + 1), V - 1)[c % 4] for c in range(G)]
            st["tseq"][P0, :] = first
            for c in range(G):    # the target's state behind its first close
                h, r = S.ts_replay(*S.ts_start(tsb, V, maxi), [first[c]], vocab)
                st["tts_hist"][c], st["tts_rng"][c] = h, r
            out = run(dbg, 0, st, G, 1, 8, vocab, tts_on, dts_on)
            ref = S.adopt_ref(lists(st), G, P0, rules_of(vocab, tts_on), rules_of(vocab, dts_on))
            same(out, st, ref, (G, tts_on, dts_on))
            assert np.array_equal(out["tseq"], st["tseq"]) and np.array_equal(out["dseq"][P0], first)
            assert np.all(out["stats"][:G] == 0)
            for k in STATE4:
                assert np.all(out[k][G:] == SENT), (G, k)                     # rows behind the group
            for k, on in (("chist", tts_on), ("crng", tts_on), ("dchist", dts_on), ("dcrng", dts_on), ("dts_hist", dts_on)):
                assert np.all(out[k][:G] != SENT) if on else np.all(out[k] == SENT), (G, k, on)
            if tts_on:
                assert np.array_equal(out["chist"][:G], st["tts_hist"][:G]) and np.array_equal(out["crng"][:G], st["tts_rng"][:G])
            if tts_on and dts_on:    # set alike, the draft's rebuilt state is the target's
                assert np.array_equal(out["dchist"], out["chist"]) and np.array_equal(out["dcrng"], out["crng"])


# ---------------------------------------------------------------- stage
def proposals(vocab, last_ts, c, w, salt):
    """w - 1 proposals that mix text, eot and rising, equal and falling timestamps (against the window's last timestamp)"""
    tsb, eot, V, _ = vocab
    base = last_ts if last_ts >= tsb else tsb + 4
    kinds = (11 + c % 50, eot, min(V - 1, base + 2), base, max(tsb, base - 3))
    return [kinds[(c + 2 * s + salt) % 5] for s in range(1, w)]


@pytest.mark.parametrize("G,w", SHAPES)
def test_stage(dbg, G, w):
    kinds = set()
    for vname, rules in (("tiny", 1), ("tiny", 0), ("production", 1)):
        vocab = VOCABS[vname]
        tsb, eot, V, _ = vocab
        hs = histories(vocab)
        start = [hs[(37 * c + 5 * G) % len(hs)] for c in range(G)]            # window c: (tokens, hist, rng)
        kinds |= {(h[1], h[2], h[3] == V - 1) for _, h, _ in start}
        for sub in "abcd":
            pos = P0 + 2 if sub != "d" else N_CTX - max(1, w // 2)            # (d): positions pos + s >= n_ctx are not staged
            g1 = pos + 1 - P0                                                 # generated index of the first proposal
            max_new = {"a": 40, "b": g1 + max(1, (w - 1) // 2), "c": 40, "d": N_CTX}[sub]
            st = fresh(G, w, max_new, pos)
            for c in range(G):
                st["chist"][c], st["crng"][c] = start[c][1], start[c][2]
            own = [proposals(vocab, start[c][1][3], c, w, 0) for c in range(G)]      # the draft's tokens
            for c in range(G):
                for s in range(1, w):
                    if pos + s < N_CTX:
                        st["dseq"][pos + s, c] = own[c][s - 1]
            d = own
            if sub in "bc":
                st["script"] = np.full((G, max_new), SENT, np.int32)
                scr = [proposals(vocab, start[c][1][3], c, w, 1) for c in range(G)]
                if sub == "c":    # ids outside the vocabulary: clamped to 0 and n_vocab - 1
                    scr = [[(-5, V + 3, t)[(c + s) % 3] for s, t in enumerate(row)] for c, row in enumerate(scr)]
                for c in range(G):
                    for s in range(1, w):
                        if g1 + s - 1 < max_new:
                            st["script"][c, g1 + s - 1] = scr[c][s - 1]
                d = [[min(max(scr[c][s - 1], 0), V - 1) if g1 + s - 1 < max_new else own[c][s - 1] for s in range(1, w)] for c in range(G)]
                if sub == "b" and w >= 3:    # the script ends inside the panel: both sources are read
                    assert g1 < max_new < g1 + w - 1 and any(d[c] != own[c] and d[c][-1] == own[c][-1] for c in range(G))
            out = run(dbg, 1, st, G, w, max_new, vocab, rules, 0)
            what = (vname, rules, sub)
            same(out, st, S.stage_ref(lists(st), G, w, P0, N_CTX, max_new, V, rules_of(vocab, rules)), what)
            # the same, from the proposals this test chose
            staged = [s for s in range(1, w) if pos + s < N_CTX]
            assert sub != "d" or len(staged) == (max(1, w // 2) - 1 if w > 1 else 0)
            changed = out["tseq"] != st["tseq"]
            assert not changed[:pos + 1].any() and not changed[pos + w:].any(), what
            for c in range(G):
                assert [int(out["tseq"][pos + s, c]) for s in staged] == d[c][:len(staged)], (what, c)
                slots = out["tts_rng"][c * w:(c + 1) * w]
                if not rules:
                    continue
                assert tuple(slots[0]) == tuple(start[c][2]), (what, c)
                for s in range(1, w):
                    want = S.ts_replay(start[c][1], start[c][2], d[c][:s], vocab)[1] if s in staged else (SENT,) * 4
                    assert tuple(slots[s]) == want, (what, c, s)
            if not rules:
                assert np.all(out["tts_rng"] == SENT), what
            assert np.all(out["tts_rng"][G * w:] == SENT), what
            for k in ("chist", "crng", "dseq", "pos2"):
                assert np.array_equal(out[k], st[k]), (what, k)
    if G >= 42:   # the start state, after text, an opening timestamp, a closed pair, the last timestamp at the top of the vocabulary
        assert {(0, 1), (0, 0), (1, 0), (1, 1)} <= {k[:2] for k in kinds} and any(k[2] for k in kinds)


# ---------------------------------------------------------------- commit
def draw_commit(rng, i, G, w, vocab):
    """case i of a shape: the state, the call's parameters and the generated index of the round's first token.  Cases 0 .. 4
    are steered: nobody live; every live window stops; everybody keeps the whole width; one window is cut short by another;
    the call's last token is the panel's last but one, so the last log-prob slot does not exist."""
    tsb, EOT, V, _ = vocab
    eot = -1 if i % 4 == 3 or i == 2 else EOT
    g0 = (0, 1, 1, 7, 20)[rng.integers(5)]                                   # 0: the first token itself is the round's
    # the call ends inside or just behind the panel, or far behind it
    max_new = g0 + int(rng.integers(1, w + 3)) if i % 5 == 4 else 40
    if i == 4:
        g0, max_new = 7, 7 + w - 1
    pos = P0 + g0 - 1
    st = fresh(G, w, max_new, pos)
    st["pos2"][1] = pos + w                                                   # the draft has taken its w steps
    st["stats"][:G] = rng.integers(0, 50, (G, 4))
    st["done"][:G] = rng.random(G) < 0.3 if G > 1 else 0
    st["acc"][:G] = rng.integers(0, w, G)
    hs = histories(vocab)
    for c in range(G):
        for hk, rk in (("chist", "crng"), ("dchist", "dcrng")):
            _, st[hk][c], st[rk][c] = hs[int(rng.integers(len(hs)))]
    # winners: text and timestamps, eot at index (i // 2 + c) % w of some windows, wherever that falls against acc
    tok = np.where(rng.random(G * w) < 0.6, rng.integers(0, EOT, G * w), rng.integers(tsb, V, G * w)).astype(np.int32)
    for c in range(G):
        if rng.random() < 0.34 or (G == 1 and i % 2 == 0):
            tok[c * w + (i // 2 + c) % w] = EOT
    st["wtok"][:G * w] = tok
    st["wlp"][:G * w] = -rng.random(G * w).astype(np.float32) - 0.25
    if i % 2 == 1:   # budgets that end in front of the panel, inside it, with it, behind it
        st["budget"] = np.full(st["acc"].shape[0], SENT, np.int32)
        st["budget"][:G] = g0 + (i // 2 + np.arange(G)) % (w + 3)
    if i == 0:
        st["done"][:G] = 1
    elif i == 1:     # eot is every live window's first token
        st["done"][:G] = np.arange(G) % 3 == 2
        st["wtok"][:G * w:w] = EOT
        st["budget"] = None
    elif i == 2:     # nothing stops anybody
        st["done"][:G], st["acc"][:G] = 0, w - 1
    elif i == 4:
        st["done"][:G], st["acc"][:G] = 0, w - 1
    elif i == 3 and G > 1:   # window 0 misses at row 0, window 1 accepts everything
        st["done"][:2], st["acc"][:2], st["budget"] = 0, (0, w - 1), None
    return st, dict(max_new=max_new, eot=eot, pad_tok=eot if eot >= 0 else 0, tts_on=int(rng.integers(2)), dts_on=int(rng.integers(2))), g0


def own_tokens(L, c, w, eot, max_new, g0):
    """spec_round.h: the tokens live window c would write if nothing but itself cut it short"""
    mine = L["wtok"][c * w:c * w + L["acc"][c] + 1]
    left = min(max_new, L["budget"][c] if L["budget"] is not None else max_new) - g0
    return S.window_own(L["acc"][c], mine.index(eot) if eot >= 0 and eot in mine else -1, left)


@pytest.mark.parametrize("G,w", SHAPES)
def test_commit_against_the_restatement(dbg, G, w):
    """40 seeded cases per shape against commit_ref, then the same stated from the cut n.  The draw's coverage is asserted at the
    end.  ("cut short by another window": a window that stays live keeps fewer tokens than its own acc + 1, n < acc[c] + 1 --
    n is never below min(acc) + 1 over the live windows, every ask being acc + 1 or nothing.)"""
    rng = np.random.default_rng(1000 * G + w)
    seen = set()
    for i in range(40):
        vocab = VOCABS["tiny" if i % 2 == 0 else "production"]
        st, par, g0 = draw_commit(rng, i, G, w, vocab)
        if i >= 4:
            par["tts_on"], par["dts_on"] = (i >> 2) & 1, (i >> 3) & 1         # every rule setting, whatever the draw
        max_new, eot, pad_tok, tts_on, dts_on = par["max_new"], par["eot"], par["pad_tok"], par["tts_on"], par["dts_on"]
        pos = int(st["pos2"][0])
        out = run(dbg, 2, st, G, w, max_new, vocab, tts_on, dts_on, eot, pad_tok)
        L = lists(st)
        ref = S.commit_ref(L, G, w, P0, N_CTX, max_new, eot, pad_tok, rules_of(vocab, tts_on), rules_of(vocab, dts_on))
        what = (i, vocab[2])
        same(out, st, ref, what)
        # the same, stated from the cut: what moved and what did not
        n = ref["tpos"] - pos
        live = [c for c in range(G) if st["done"][c] == 0]
        assert out["pos2"].tolist() == [pos + n, pos + n] and out["round"].tolist() == [int(out["n_live"][0]), pos + n], what
        assert out["n_live"][0] == sum(1 for c in range(G) if out["done"][c] == 0), what
        changed = out["tseq"] != st["tseq"]
        assert not changed[:pos + 1].any() and not changed[pos + 1 + n:].any() and np.all(out["tseq"][pos + 1:pos + 1 + n] >= 0), what
        rows = sorted(set(np.nonzero(out["dseq"] != st["dseq"])[0].tolist()))
        assert rows == ([pos + n] if n else []) and (n == 0 or np.array_equal(out["dseq"][pos + n], out["tseq"][pos + n])), what
        written = as_int(out["logprob"]) != SENT_F32
        assert np.array_equal(np.nonzero(written.all(axis=1))[0], np.arange(g0, min(g0 + n, max_new))) and written.all(axis=1).sum() == written.any(axis=1).sum(), what
        for c in range(G):
            if c not in live:    # a frozen window: padding, nothing else
                assert out["tseq"][pos + 1:pos + 1 + n, c].tolist() == [pad_tok] * n and np.array_equal(out["stats"][c], st["stats"][c]), (what, c)
                assert out["done"][c] == st["done"][c], (what, c)
        if tts_on:
            for c in range(G):    # the committed state: behind the m tokens the window kept, untouched when it kept none
                m = min(n, own_tokens(L, c, w, eot, max_new, g0)) if c in live else 0
                h, r = S.ts_replay(L["chist"][c], L["crng"][c], out["tseq"][pos + 1:pos + 1 + m, c].tolist(), vocab)
                assert (tuple(out["chist"][c]), tuple(out["crng"][c])) == (h, r), (what, c)
                assert m > 0 or (np.array_equal(out["chist"][c], st["chist"][c]) and np.array_equal(out["crng"][c], st["crng"][c])), (what, c)
                assert out["tseq"][pos + 1:pos + 1 + n, c].tolist() == L["wtok"][c * w:c * w + m] + [pad_tok] * (n - m), (what, c)
        else:
            assert np.array_equal(out["chist"], st["chist"]) and np.array_equal(out["crng"], st["crng"]), what
        if dts_on:
            for c in range(G):
                h, r = S.ts_replay(L["dchist"][c], L["dcrng"][c], out["tseq"][pos + 1:pos + 1 + n, c].tolist(), vocab)
                for hk, rk in (("dchist", "dcrng"), ("dts_hist", "dts_rng")):
                    assert (tuple(out[hk][c]), tuple(out[rk][c])) == (h, r), (what, c, hk)
        else:
            for k in ("dchist", "dcrng", "dts_hist", "dts_rng"):
                assert np.array_equal(out[k], st[k]), (what, k)
        # what this case covered
        seen.add(("n", 0 if n == 0 else w if n == w else -1))
        if live and out["n_live"][0] == 0:
            seen.add("all stop")
        if any(n < st["acc"][c] + 1 and out["done"][c] == 0 for c in live):
            seen.add("cut short by another window")
        if live and len(live) < G:
            seen.add("frozen beside live")
        seen.add(("eot", eot >= 0))
        seen.add(("rules", tts_on, dts_on))
        seen.add(("g0", min(g0, 2)))
        if st["budget"] is None:
            seen.add("no budget")
        else:
            for c in live:
                b = int(st["budget"][c]) - g0
                seen.add(("budget", "before" if b <= 0 else "inside" if b < w else "at" if b == w else "behind"))
        if eot >= 0:
            seen |= {("eot at", j) for c in live for j in range(w) if st["wtok"][c * w + j] == eot}
        if max_new < g0 + n:
            seen.add("log-probs end at max_new")
    need = {("n", 0), ("n", w), "all stop", ("eot", False), ("eot", True), "no budget", ("g0", 0), ("g0", 1), ("g0", 2),
            ("budget", "before"), ("budget", "at"), ("budget", "behind"), "log-probs end at max_new"}
    need |= {("rules", a, b) for a in (0, 1) for b in (0, 1)} | {("eot at", j) for j in range(w)}
    if w > 1:
        need |= {("n", -1), ("budget", "inside")}
    if G > 1:
        need |= {"frozen beside live"} | ({"cut short by another window"} if w > 1 else set())
    assert need <= seen, sorted(map(str, need - seen))


# ---------------------------------------------------------------- adopt, then rounds of stage -> commit
def test_rounds_chained(dbg):
    """5 windows x 4 rows, rules on both sides, 8 rounds.  Each window has its own token stream (what the target would choose);
    the proposals are that stream but for the MISSES below, the winners are the stream up to the first miss and something else
    behind it.  Window 3 ends with eot at generated index 5, window 4 is frozen from the start.  After every round the committed
    state of window c is ts_start advanced along the tokens it has kept so far -- whatever the staging replayed along rejected
    proposals in between -- and the next staging starts from it."""
    vocab = VOCABS["tiny"]
    tsb, eot, V, maxi = vocab
    G, w, max_new = 5, 4, 40

    def stream(c):    # <|t|> text text <|t'|><|t'|> text text ...
        out, t = [tsb + c], tsb + c
        while len(out) < max_new:
            t += 2 + c
            out += [30 + c + len(out), 60 + c + len(out), t, t]
        return out[:max_new]
    truth = [stream(c) for c in range(G)]
    truth[3][5] = eot
    # (round, window): the proposal that is wrong and what it is -- in round order a miss at proposal 0, 1 and w - 2 (the last
    # one a panel has), timestamps where text was right and the reverse
    MISSES = {(0, 0): (0, V - 2), (1, 1): (1, 611), (2, 2): (2, tsb + 60), (4, 0): (2, 612), (4, 1): (0, tsb + 90), (6, 2): (1, eot)}
    WANT_N = [1, 2, 3, 4, 1, 4, 2, 4]                                         # by hand, from MISSES
    WANT_ACC = [[0, 3, 3], [3, 1, 3], [3, 3, 2], [3, 3, 3], [2, 0, 3], [3, 3, 3], [3, 3, 1], [3, 3, 3]]   # windows 0 .. 2
    st = fresh(G, w, max_new, P0)
    st["tseq"][P0] = [truth[c][0] for c in range(G)]
    for c in range(G):
        st["tts_hist"][c], st["tts_rng"][c] = S.ts_replay(*S.ts_start(tsb, V, maxi), truth[c][:1], vocab)
    out = run(dbg, 0, st, G, 1, max_new, vocab, 1, 1)
    same(out, st, S.adopt_ref(lists(st), G, P0, vocab, vocab), "adopt")
    # the adoption ran at width 1: the per-row arrays of a round of width w
    st = dict(out, tts_rng=np.full_like(fresh(G, w, max_new, P0)["tts_rng"], SENT), wtok=np.full((G + 3) * w, SENT, np.int32),
              wlp=np.full((G + 3) * w, SENT_F32, np.uint32).view(np.float32))
    st["done"][:G] = [0, 0, 0, 0, 1]
    kept = [truth[c][:1] for c in range(G)]                                   # the tokens a window has kept
    stopped_mid_panel = False
    for rnd in range(8):
        pos = int(st["pos2"][0])
        g0 = pos + 1 - P0
        # the draft's w - 1 tokens
        d = [[truth[c][g0 + s] for s in range(w - 1)] for c in range(G)]
        for c in range(G):
            if (rnd, c) in MISSES:
                d[c][MISSES[rnd, c][0]] = MISSES[rnd, c][1]
        for c in range(G):
            st["dseq"][pos + 1:pos + w, c] = d[c]
        st["pos2"][1] = pos + w
        out = run(dbg, 1, st, G, w, max_new, vocab, 1, 1)
        same(out, st, S.stage_ref(lists(st), G, w, P0, N_CTX, max_new, V, vocab), ("stage", rnd))
        for c in range(G):    # the staging starts from the committed state: the tokens kept so far, nothing a rejected proposal left
            want = S.ts_replay(*S.ts_start(tsb, V, maxi), kept[c], vocab)
            assert (tuple(out["chist"][c]), tuple(out["crng"][c])) == want and tuple(out["tts_rng"][c * w]) == want[1], (rnd, c)
            assert tuple(out["tts_rng"][c * w + w - 1]) == S.ts_replay(*want, d[c], vocab)[1], (rnd, c)
        st = out
        # the verify step: the window's own choice while the proposals in front of a row were right, another token behind that
        acc = [next((s for s in range(w - 1) if d[c][s] != truth[c][g0 + s]), w - 1) for c in range(G)]
        for c in range(G):
            st["wtok"][c * w:(c + 1) * w] = [truth[c][g0 + s] if s <= acc[c] else 700 + s for s in range(w)]
        st["acc"][:G] = acc
        st["wlp"][:G * w] = -(np.arange(G * w, dtype=np.float32) + 1) / 64 - rnd
        assert acc[:3] == WANT_ACC[rnd], (rnd, acc)
        live = [c for c in range(G) if st["done"][c] == 0]
        out = run(dbg, 2, st, G, w, max_new, vocab, 1, 1, eot, eot)
        same(out, st, S.commit_ref(lists(st), G, w, P0, N_CTX, max_new, eot, eot, vocab, vocab), ("commit", rnd))
        n = int(out["pos2"][0]) - pos
        assert n == WANT_N[rnd], (rnd, n)
        for c in live:
            own = truth[c][g0:g0 + n]
            if eot in own:
                stopped_mid_panel |= own.index(eot) < n - 1
                own = own[:own.index(eot) + 1]
            kept[c] = kept[c] + own
        for c in range(G):
            col = out["tseq"][P0:pos + n + 1, c].tolist()
            assert col == kept[c] + [eot] * (len(col) - len(kept[c])), (rnd, c)
            # the rollback: the committed state is the kept tokens' -- not the proposals' that the staging replayed
            want = S.ts_replay(*S.ts_start(tsb, V, maxi), kept[c], vocab)
            assert (tuple(out["chist"][c]), tuple(out["crng"][c])) == want, (rnd, c)
            # the draft's: along everything the group's buffer holds, a finished window's padding included
            dwant = S.ts_replay(*S.ts_start(tsb, V, maxi), col, vocab)
            assert (tuple(out["dchist"][c]), tuple(out["dcrng"][c])) == dwant == (tuple(out["dts_hist"][c]), tuple(out["dts_rng"][c])), (rnd, c)
        assert out["done"][:G].tolist() == [0, 0, 0, int(eot in kept[3]), 1], rnd
        st = out
    assert stopped_mid_panel and len(kept[4]) == 1 and kept[3][-1] == eot and len(kept[3]) == 6
    assert st["stats"][:G, 0].tolist() == [8, 8, 8, 3, 0]
