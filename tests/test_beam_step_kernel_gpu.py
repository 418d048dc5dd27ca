"""Kernel-level GPU tests of a beam group's step (csrc/beam.hip beam_select_kernel), driven alone on caller-given state through
wmdbg_beam_step (include/whisper_mi355x_debug.h): the lists are the test's, no logits and no list kernel in front.  The right
answer is exact: every in / out buffer of the launch is compared WHOLE, integers and raw float bits, with the plain restatement
tests/beam_step_ref.py (select_step, reorder), which tests/test_beam_step_cpu.py holds to BeamWindowNp first.  Every buffer goes
in pre-filled with a sentinel (ints SENT, floats the NaN bits WMDBG_SENTINEL_F32, the token buffer a different negative value
per cell) and per-window / per-row arrays carry two windows behind the group's: "nothing else was written" is part of every
comparison.  Only the bf16 copy, the statistics and the mean of the embedded row have bounds: check_embedding's, as they are.

n_ctx = 24, n_vocab = 96 (eot 70, timestamps from 80), max_new 16, d 64 / 576 (576: columns beyond the 512 a wave keeps in
registers).  One 1024-thread workgroup per launch: wave v takes windows v, v + 16, v + 32, ... through one LDS slot.

MEASURED on the MI355X: every case passes with the kernel as it is (no defect found); the file takes 3.0 s, no case more than
0.1 s (a whole search: 16 select + 16 re-parenting launches in 0.05 - 0.07 s).  Three deliberately wrong kernels, each built
into a scratch debug library and run against this file: the inherited rule state read from hist_s[wave][lane] fails
test_timestamp_state_follows_the_source_beam, the rules-on draw of test_one_step_every_field and every whole search; the
finished history read from row0 + f instead of the source beam fails test_one_step_every_field, the whole searches and every
test that compares the finished records; n_from = N at generated index 0 fails test_one_step_every_field and every whole search."""
import ctypes
import functools
import types

import numpy as np
import pytest

import beam_step_ref as R
import spec_ref as S
from test_beam_step_cpu import BeamIo, bits, drive_windows, same_hypotheses
from test_decode_step_kernels_gpu import bf, check_embedding

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
f32 = np.float32
WM_ERR_INVALID = 1
N_CTX, P0, V, MAX_NEW, EOT, N_TEXT, TS = R.N_CTX, R.N_PROMPT, R.N_VOCAB, R.MAX_NEW, R.EOT, R.N_TEXT, R.TS
SENT, SENT32, SENT16 = R.SENT, R.SENT_F32, 0x7fc5
HOST_FILL = f32(0.25)                          # what the embedding outputs hold on the host before a call
STATE = ("budget", "sum", "list_n", "list_tok", "list_lp", "src", "wdone", "wsteps", "fin_n", "fin_len", "fin_sum", "fin_src", "fin_tok",
         "fin_lp", "anc", "seq", "logprob", "hist", "rng", "done", "live_rows", "n_live", "off")
POOL = np.array(list(range(N_TEXT)) + list(range(TS[0], V)))      # the lists' tokens: text and timestamps (eot = N_TEXT is drawn apart)
GEOMS = [(1, 1), (1, 8), (16, 8), (17, 7), (33, 3), (128, 1), (25, 5)]


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_beam_step.argtypes = [vp, ctypes.POINTER(BeamIo)]
    c.lib.wmdbg_beam_reorder.argtypes = [vp, vp] + [ctypes.c_int] * 7 + [vp, vp, vp, vp]
    lay = (ctypes.c_int32 * 4)()      # the ctypes restatement against the header's struct
    assert c.lib.wmdbg_beam_step_layout(lay) == 0
    assert list(lay) == [ctypes.sizeof(BeamIo), BeamIo.ts_par.offset, BeamIo.budget.offset, BeamIo.x_next.offset], list(lay)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def world(d):
    """the embedding tables of one width, shared and never modified"""
    rng = np.random.default_rng(d)
    w = types.SimpleNamespace(K=d)
    w.emb = bf(rng.standard_normal((V, d)) * (2.0 / np.sqrt(d)) + np.linspace(-0.02, 0.02, d)[None, :] + np.linspace(-0.01, 0.01, V)[:, None])
    w.pemb = (rng.standard_normal((N_CTX, d)) * 0.3 + 1.0).astype(f32)     # (a mean of 1: a row's sum does not cancel)
    return w


def ib(a):
    """an array as integers: floats by their bits"""
    return bits(a) if a.dtype == f32 else a


def run(dbg, st, C, N, pos, par, *, d=64, ts=None, stop=False, n_prompt=P0, n_ctx=N_CTX, n_vocab=V, cap=None, expect_ok=True):
    """one wmdbg_beam_step call on copies of st's arrays -> the state behind it, with the embedding outputs and the return code"""
    out = {k: (None if st.get(k) is None else np.ascontiguousarray(st[k]).copy()) for k in STATE}
    w = world(d if d in (64, 576) else 64)
    nr = out["sum"].shape[0]
    dd = max(d, 1)
    out.update(x_next=np.full((nr, dd), HOST_FILL, f32), xb_next=np.full((nr, dd), HOST_FILL, f32), stats_next=np.full((nr, 2), HOST_FILL, f32),
               mean_next=np.full(nr, HOST_FILL, f32))
    io = BeamIo()
    io.C, io.N, io.cap = C, N, out["wdone"].shape[0] if cap is None else cap
    io.n_ctx, io.pos, io.n_prompt, io.d, io.n_vocab = n_ctx, pos, n_prompt, d, n_vocab
    io.max_cand, io.max_new, io.eot, io.pad = par
    io.ts_on, io.stop_on = int(ts is not None), int(stop)
    io.ts_par[:] = ts if ts is not None else (0, 0, 0, 0)
    for k, v in out.items():
        setattr(io, k, None if v is None else v.ctypes.data_as(vp))
    io.emb, io.pemb = w.emb.ctypes.data_as(vp), w.pemb.ctypes.data_as(vp)
    io.stats_tail_nonzero = io.pos_out = SENT
    out["rc"] = dbg.lib.wmdbg_beam_step(dbg.handle, ctypes.byref(io))
    if expect_ok:
        assert out["rc"] == 0, dbg.lib.wm_last_error()
    out["tail"], out["pos_out"] = io.stats_tail_nonzero, io.pos_out
    return out


def same(out, want, what):
    """every in / out array behind the launch equals the restatement's: what it wrote where it wrote, the input everywhere else"""
    for k in STATE:
        if want.get(k) is None:
            assert out[k] is None, (what, k)
            continue
        assert out[k].shape == want[k].shape and np.array_equal(ib(out[k]), ib(want[k])), (what, k, np.argwhere(ib(out[k]) != ib(want[k]))[:4])


def embedding(out, info, C, N, pos, d, off=None, n_ctx=N_CTX):
    """the embedded rows as check_embedding checks them (exact f32 bits for x, its bounds for the bf16 copy and the statistics),
    the mean at the statistics' rtol, and the sentinels of the rows behind the group's"""
    rows = C * N
    r = types.SimpleNamespace(B=rows, x_next=out["x_next"][:rows], xb_next=out["xb_next"][:rows], stats=out["stats_next"][:rows], tail=out["tail"])
    check_embedding(world(d), r, info["tok"], pos, n_ctx, off)
    assert np.all(bits(out["x_next"][rows:]) == SENT32) and np.all(bits(out["xb_next"][rows:]) == SENT16 << 16)
    assert np.all(bits(out["mean_next"][rows:]) == SENT32)
    if pos + 1 >= n_ctx:
        assert not info["embedded"] and np.all(bits(out["mean_next"]) == SENT32)
        return
    want = R.embed_x(world(d).emb, world(d).pemb, info["tok"], info["prow"])
    assert np.array_equal(bits(out["x_next"][:rows]), bits(want))
    assert np.allclose(out["mean_next"][:rows], want.astype(np.float64).mean(axis=1), rtol=1e-5, atol=0)


def random_state(seed, C, N, gi, max_cand, *, anc=True, ts=None, eot=EOT, n_prompt=P0, n_ctx=N_CTX, p_done=0.2, p_dead=0.15):
    """A group in front of generated index gi: distinct history cells (a wrong source row shows), random sums with dead beams,
    windows that have left, finished counts up to max_cand, budgets at, above and below gi + 1, random lists with eot, short and
    empty ones, score ties.  At gi == 0 beam 0 has the WORST sum: the others must not contribute."""
    rng = np.random.default_rng(seed)
    rows, pos = C * N, n_prompt - 1 + gi
    st = R.fresh(C, N, C + 2, n_ctx, MAX_NEW, anc)
    st["seq"][:pos + 1] = 100 + np.arange((pos + 1) * rows).reshape(pos + 1, rows)
    st["logprob"][:gi] = (-(1 + np.arange(gi * rows)) / 64.0).astype(f32).reshape(gi, rows)
    st["budget"][:C] = rng.choice([gi + 1, gi + 2, MAX_NEW, max(1, gi)], size=C)
    st["wdone"][:C] = rng.random(C) < p_done
    st["wdone"][0] = 0
    st["wsteps"][:C] = np.where(st["wdone"][:C] != 0, rng.integers(0, gi + 1, size=C), gi)
    st["fin_n"][:C] = np.minimum(rng.integers(0, max_cand + 2, size=C), max_cand)
    sums = (np.round(-rng.exponential(3.0, size=rows) * 2) / 2).astype(f32)
    sums[rng.random(rows) < p_dead] = -np.inf
    if gi == 0:
        sums.reshape(C, N)[:, 0] = -9.0
        sums.reshape(C, N)[:, 1:] = -0.125
    st["sum"][:rows] = sums
    for w in range(C):
        R.put_lists(st, w * N, R.random_lists(rng, N, POOL, eot if eot >= 0 else EOT, 0.4, 0.3, 0.5 if w % 3 == 0 else 0.0))
    if ts is not None:
        hs = histories()
        for b in range(rows):
            _, st["hist"][b], st["rng"][b] = hs[int(rng.integers(0, len(hs)))]
    return st, pos


@functools.lru_cache(maxsize=None)
def histories():
    """every history of up to 4 tokens the rules allow over text, eot and four timestamps: (tokens, hist, rng)"""
    hs, _ = S.rule_histories((5, 17, EOT, TS[0], TS[0] + 1, TS[0] + 7, V - 1), TS, 4)
    return hs


# ---------------------------------------------------------------- 1. one step, every field
@pytest.mark.parametrize("C,N", GEOMS)
def test_one_step_every_field(dbg, C, N):
    """Generated index 0 (beam 0 alone, whatever the others' sums) and 5, three draws each, ancestry and rules on and off; windows 16 .. 31
    take a wave's second trip through its LDS slot, 32 and above the third."""
    rows = C * N
    fins = forks = 0
    for gi in (0, 5):
        for draw in range(3):
            anc, ts = draw != 1, (TS if draw == 2 else None)
            max_cand = (N, 1, 16)[draw]
            st, pos = random_state(7000 * C + 100 * N + 10 * gi + draw, C, N, gi, max_cand, anc=anc, ts=ts)
            par = (max_cand, MAX_NEW, EOT, EOT)
            want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, ts, True)
            out = run(dbg, st, C, N, pos, par, ts=ts, stop=True)
            what = (C, N, gi, draw)
            same(out, want, what)
            assert out["pos_out"] == pos + 1 == info["pos"], what
            embedding(out, info, C, N, pos, 64)
            # said once more without the restatement: the outputs of the contract, and that the rest is untouched
            assert np.array_equal(out["seq"][:pos + 1], st["seq"][:pos + 1]) and np.array_equal(out["seq"][pos + 2:], st["seq"][pos + 2:])
            assert np.array_equal(bits(out["logprob"][:gi]), bits(st["logprob"][:gi])) and np.all(bits(out["logprob"][gi + 1:]) == SENT32)
            assert np.all(out["seq"][pos + 1] >= 0) and np.all(bits(out["logprob"][gi]) != SENT32)
            for k in ("sum", "list_lp"):
                assert np.all(bits(out[k][rows:]) == SENT32), (what, k)
            for k in ("src", "list_n", "done", "hist", "rng", "wdone", "wsteps", "fin_n", "fin_len", "fin_tok", "fin_src"):
                n = rows if out[k].shape[0] == (C + 2) * N else C
                assert np.all(out[k][n:] == SENT), (what, k)
            if ts is None:
                assert np.all(out["hist"] == SENT) and np.all(out["rng"] == SENT)        # rules off
            if anc:
                assert np.array_equal(out["anc"][gi], out["src"][:rows]) and np.all(np.delete(out["anc"], gi, axis=0) == SENT)
            else:
                assert np.all(out["fin_src"] == SENT)
            for w in range(C):
                r = slice(w * N, (w + 1) * N)
                if st["wdone"][w]:
                    continue
                f0, f1 = int(st["fin_n"][w]), int(out["fin_n"][w])
                assert f0 <= f1 <= max_cand and int(out["wsteps"][w]) == gi + 1
                assert int(out["wdone"][w]) == int(f1 >= max_cand or gi + 1 >= st["budget"][w])
                if gi == 0:
                    assert np.all(out["src"][r][out["sum"][r] != -np.inf] == 0), what      # beam 0 alone contributes
                forks += not np.array_equal(out["src"][r], np.arange(N))
                for s in range(f0, f1):      # a finished hypothesis: the SOURCE beam's history, then eot
                    fins += 1
                    assert int(out["fin_len"][w, s]) == gi + 1 and int(out["fin_tok"][w, s, gi]) == EOT
                    if anc:
                        j = w * N + int(out["fin_src"][w, s])
                        assert np.array_equal(out["fin_tok"][w, s, :gi], st["seq"][P0:P0 + gi, j])
                        assert np.array_equal(bits(out["fin_lp"][w, s, :gi]), bits(st["logprob"][:gi, j]))
                assert np.all(out["fin_len"][w, :f0] == SENT) and np.all(out["fin_len"][w, f1:] == SENT)
                assert np.all(out["fin_tok"][w, f1:] == SENT) and np.all(bits(out["fin_lp"][w, f1:]) == SENT32)
    if C >= 16:
        assert fins >= 2 and (N == 1 or forks >= 2), (fins, forks)


# ---------------------------------------------------------------- 2. the timestamp state follows the source beam
@pytest.mark.parametrize("N", [2, 5])
def test_timestamp_state_follows_the_source_beam(dbg, N):
    """The beams of a window stand behind different histories (an open timestamp, a closed pair, text); the lists force src to
    be a rotation (windows 0, 3), all from one beam (1, 4) and whatever a random draw gives (5 ..); window 2 has left."""
    C, gi = 19, 3
    rows, pos = C * N, P0 - 1 + 3
    hs = histories()
    kinds = [[h for h in hs if h[1][0] >= 2 and h[1][1] == 1 and h[1][2] == 0],       # an open timestamp
             [h for h in hs if h[1][0] >= 2 and h[1][1] == 1 and h[1][2] == 1],       # a closed pair
             [h for h in hs if h[1][0] >= 2 and h[1][1] == 0]]                        # text last
    assert all(len(k) >= 5 for k in kinds)
    st, _ = random_state(900 + N, C, N, gi, 4, ts=TS, p_done=0.0, p_dead=0.0)
    for b in range(rows):
        _, st["hist"][b], st["rng"][b] = kinds[(b + b // N) % 3][(7 * b) % 5]
    toks = (5, TS[0] + 2, 17, TS[0] + 9, V - 1, 33, TS[0], 41)                        # text and timestamps, by beam
    for w in (0, 3):      # a rotation: beam j's one candidate has score -((j - 1) % N) - 0.5
        st["sum"][w * N:(w + 1) * N] = [-((j - 1) % N) for j in range(N)]
        R.put_lists(st, w * N, [[(toks[j + w], f32(-0.5))] for j in range(N)])
    for w, b in ((1, N - 1), (4, 0)):      # all from beam b: the others' sums lie far below
        st["sum"][w * N:(w + 1) * N] = [-1.0 if j == b else -200.0 for j in range(N)]
        R.put_lists(st, w * N, [[(toks[(e + j) % 8], f32(-0.25 * (e + 1))) for e in range(N + 1)] for j in range(N)])
    st["wdone"][2] = 1
    for w in (0, 1, 3, 4):
        st["budget"][w], st["fin_n"][w] = MAX_NEW, 0
    par = (4, MAX_NEW, EOT, EOT)
    want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, TS, True)
    out = run(dbg, st, C, N, pos, par, ts=TS, stop=True)
    same(out, want, N)
    for w in (0, 3):
        assert out["src"][w * N:(w + 1) * N].tolist() == [(k + 1) % N for k in range(N)]
    assert out["src"][N:2 * N].tolist() == [N - 1] * N and out["src"][4 * N:5 * N].tolist() == [0] * N
    moved = 0
    for b in range(rows):      # said without the restatement: (hist, rng) = ts_advance(hist[src], token)
        w = b // N
        if w == 2:
            assert np.array_equal(out["hist"][b], st["hist"][b]) and np.array_equal(out["rng"][b], st["rng"][b])
            continue
        a = w * N + int(out["src"][b])
        h, g = S.ts_advance(tuple(int(v) for v in st["hist"][a]), int(out["seq"][pos + 1, b]), TS[0], TS[1], TS[2])
        assert out["hist"][b].tolist() == list(h) and out["rng"][b].tolist() == list(g), b
        h2, g2 = S.ts_advance(tuple(int(v) for v in st["hist"][b]), int(out["seq"][pos + 1, b]), TS[0], TS[1], TS[2])
        moved += (h, g) != (h2, g2)
    assert moved >= 8          # the slot's own history would have given another state: the test can tell the two apart
    assert np.all(out["hist"][rows:] == SENT) and np.all(out["rng"][rows:] == SENT)
    # rules off: both buffers keep their sentinel
    st["hist"][:], st["rng"][:] = SENT, SENT
    want, _ = R.select_step(st, C, N, pos, P0, N_CTX, par, None, True)
    out = run(dbg, st, C, N, pos, par, stop=True)
    same(out, want, (N, "rules off"))
    assert np.all(out["hist"] == SENT) and np.all(out["rng"] == SENT)


# ---------------------------------------------------------------- 3. leaving and padding
def leaving_state(eot):
    C, N, gi = 6, 3, 4
    st = R.fresh(C, N, C + 2, N_CTX, MAX_NEW, True)
    rows, pos = C * N, P0 - 1 + gi
    st["seq"][:pos + 1] = 100 + np.arange((pos + 1) * rows).reshape(pos + 1, rows)
    st["logprob"][:gi] = (-(1 + np.arange(gi * rows)) / 64.0).astype(f32).reshape(gi, rows)
    st["wdone"][:C], st["wsteps"][:C], st["fin_n"][:C], st["budget"][:C] = 0, gi, 0, MAX_NEW
    st["sum"][:rows] = (-1 - np.arange(rows) % N).astype(f32)
    plain = lambda w: [[(10 + 3 * j + e + w, f32(-0.5 * (e + 1))) for e in range(N + 1)] for j in range(N)]
    for w in range(C):
        R.put_lists(st, w * N, plain(w))
    # window 0 has left: recognisable sums, counts and steps that must stay
    st["wdone"][0], st["wsteps"][0], st["fin_n"][0] = 1, 2, 1
    # window 1 reaches max_cand = 4 exactly: three finished, one eot on top
    st["fin_n"][1] = 3
    R.put_lists(st, N, [[(EOT, f32(-0.125))] + plain(1)[0][:N]] + plain(1)[1:])
    # window 2 leaves by its budget, window 3 by neither (one more token allowed)
    st["budget"][2], st["budget"][3] = gi + 1, gi + 2
    # window 4: a dead beam in front (its list is ignored), two candidates for three slots: slot 2 dies, its siblings live
    st["sum"][4 * N:5 * N] = [-1.0, -np.inf, -2.0]
    R.put_lists(st, 4 * N, [[(21, f32(-0.5))], [(22, f32(-0.01)), (23, f32(-0.02))], [(24, f32(-0.5))]])
    # window 5: eot in two lists, four candidates in all
    R.put_lists(st, 5 * N, [[(EOT, f32(-0.25)), (31, f32(-0.5))], [(34, f32(-0.125)), (EOT, f32(-0.25))], []])
    return st, C, N, gi, pos


def test_leaving_and_padding(dbg):
    st, C, N, gi, pos = leaving_state(EOT)
    par = (4, MAX_NEW, EOT, EOT)
    want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, None, True)
    out = run(dbg, st, C, N, pos, par, stop=True)
    same(out, want, "leaving")
    r = lambda w: slice(w * N, (w + 1) * N)
    # window 0: pad, log-prob 0, identity src / anc, done; sums, finished records and steps untouched
    assert out["seq"][pos + 1, r(0)].tolist() == [EOT] * N and bits(out["logprob"][gi, r(0)]).tolist() == [0] * N
    assert out["src"][r(0)].tolist() == [0, 1, 2] == out["anc"][gi, r(0)].tolist() and out["done"][r(0)].tolist() == [1] * N
    assert np.array_equal(bits(out["sum"][r(0)]), bits(st["sum"][r(0)])) and (int(out["wsteps"][0]), int(out["fin_n"][0]), int(out["wdone"][0])) == (2, 1, 1)
    assert np.all(out["fin_len"][0] == SENT) and np.all(out["fin_tok"][0] == SENT) and np.all(bits(out["fin_sum"][0]) == SENT32)
    # leaves: max_cand exactly reached, gi + 1 == budget, neither
    assert (int(out["fin_n"][1]), int(out["wdone"][1])) == (4, 1) and int(out["fin_len"][1, 3]) == gi + 1 and out["done"][r(1)].tolist() == [1] * N
    assert (int(out["fin_n"][2]), int(out["wdone"][2])) == (0, 1) and out["done"][r(2)].tolist() == [1] * N
    assert (int(out["fin_n"][3]), int(out["wdone"][3])) == (0, 0) and out["done"][r(3)].tolist() == [0] * N
    assert [int(out["wsteps"][w]) for w in range(1, C)] == [gi + 1] * (C - 1)
    # a dead beam of a live window is done, its siblings are not
    assert out["seq"][pos + 1, r(4)].tolist() == [21, 24, EOT] and out["src"][r(4)].tolist() == [0, 2, 2]
    assert bits(out["sum"][r(4)]).tolist() == bits(np.array([-1.5, -2.5, -np.inf], f32)).tolist()
    assert out["done"][r(4)].tolist() == [0, 0, 1] and int(out["wdone"][4]) == 0
    # window 5: two finish in one step (scores -1.25 of beam 0, -2.25 of beam 1), in walk order
    assert int(out["fin_n"][5]) == 2 and out["fin_src"][5, :2].tolist() == [0, 1]
    assert bits(out["fin_sum"][5, :2]).tolist() == bits(np.array([-1.25, -2.25], f32)).tolist()
    assert np.array_equal(out["fin_tok"][5, 1, :gi], st["seq"][P0:P0 + gi, 5 * N + 1])
    assert out["live_rows"][:int(out["n_live"][0])].tolist() == [b for b in range(C * N) if out["done"][b] == 0]
    # eot < 0: nothing finishes, the id is an ordinary token
    par = (4, MAX_NEW, -1, 0)
    want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, None, True)
    out = run(dbg, st, C, N, pos, par, stop=True)
    same(out, want, "eot < 0")
    assert np.array_equal(out["fin_n"], st["fin_n"]) and np.all(out["fin_len"] == SENT) and np.all(out["fin_tok"] == SENT)
    assert out["seq"][pos + 1, r(1)][0] == EOT and out["seq"][pos + 1, r(0)].tolist() == [0] * N      # (pad = 0)
    assert int(out["wdone"][1]) == 0 and int(out["wdone"][2]) == 1


def test_the_last_slot_of_the_store(dbg):
    """max_cand = WM_MAX_BEAM_HYPS with 15 finished and three eot candidates: one is kept, in slot 15; the slot behind the
    store -- slot 0 of the next window's records -- is untouched."""
    C, N, gi = 1, 3, 2
    pos = P0 - 1 + gi
    st = R.fresh(C, N, 3, N_CTX, MAX_NEW, True)
    st["seq"][:pos + 1] = 100 + np.arange((pos + 1) * N).reshape(pos + 1, N)
    st["logprob"][:gi] = (-(1 + np.arange(gi * N)) / 64.0).astype(f32).reshape(gi, N)
    st["wdone"][0], st["wsteps"][0], st["fin_n"][0], st["budget"][0] = 0, gi, 15, MAX_NEW
    st["sum"][:N] = [-1, -2, -3]
    R.put_lists(st, 0, [[(EOT, f32(-0.5)), (11, f32(-1))], [(EOT, f32(-0.25)), (12, f32(-1))], [(EOT, f32(-0.125)), (13, f32(-1))]])
    par = (16, MAX_NEW, EOT, EOT)
    want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, None, False)
    assert info["events"][0] == {"eot_dropped", "leaves_by_max_cand"}
    out = run(dbg, st, C, N, pos, par)
    same(out, want, "slot 15")
    assert int(out["fin_n"][0]) == 16 and int(out["wdone"][0]) == 1 and int(out["fin_src"][0, 15]) == 0
    assert out["fin_tok"][0, 15, :gi + 1].tolist() == st["seq"][P0:P0 + gi, 0].tolist() + [EOT]
    assert np.all(out["fin_len"][0, :15] == SENT) and np.all(out["fin_len"][1:] == SENT) and np.all(out["fin_tok"][1:] == SENT)
    assert np.all(bits(out["fin_sum"][1:]) == SENT32) and np.all(bits(out["fin_lp"][1:]) == SENT32) and np.all(out["fin_src"][1:] == SENT)
    assert out["seq"][pos + 1].tolist() == [11, 12, 13]


# ---------------------------------------------------------------- 4. the live list
@pytest.mark.parametrize("C,N", [(25, 5), (16, 8), (128, 1)])
def test_live_list(dbg, C, N):
    """125 and 128 rows: the list crosses the 64-row ballot boundary, with done rows in front of it and live rows behind it."""
    rows, gi = C * N, 6
    st, pos = random_state(400 + C, C, N, gi, 3, p_done=0.3, p_dead=0.25)
    par = (3, MAX_NEW, EOT, EOT)
    want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, None, True)
    out = run(dbg, st, C, N, pos, par, stop=True)
    same(out, want, (C, N))
    n = int(out["n_live"][0])
    live = [b for b in range(rows) if out["done"][b] == 0]
    assert set(out["done"][:rows].tolist()) == {0, 1} and out["live_rows"][:n].tolist() == live and np.all(out["live_rows"][n:] == -1)
    assert any(b >= 64 for b in live) and any(b < 64 for b in live) and any(out["done"][b] for b in range(64)) and 0 < n < rows
    for w in range(C):      # done as the contract says
        for k in range(N):
            b = w * N + k
            assert int(out["done"][b]) == int(bool(out["wdone"][w]) or out["sum"][b] == -np.inf or bool(st["wdone"][w])), b
    # early stop off: done, live_rows and n_live are untouched
    want, _ = R.select_step(st, C, N, pos, P0, N_CTX, par, None, False)
    out = run(dbg, st, C, N, pos, par, stop=False)
    same(out, want, (C, N, "stop off"))
    assert np.all(out["done"] == SENT) and np.all(out["live_rows"] == -1) and int(out["n_live"][0]) == SENT


# ---------------------------------------------------------------- 5. the embedding
@pytest.mark.parametrize("d", [64, 576])
def test_embedding_of_the_next_row(dbg, d):
    """The row every beam embeds for position pos + 1 -- the pad of windows that have left and of dead beams included -- with the
    prompt starts NULL and ragged (one row starts behind pos + 1: positional row 0); at pos + 1 == n_ctx nothing is embedded and
    every other output is written."""
    for C, N in ((17, 7), (25, 5)):
        rows, gi = C * N, 4
        st, pos = random_state(50 + C + d, C, N, gi, N, p_done=0.25)
        par = (N, MAX_NEW, EOT, EOT)
        for ragged in (False, True):
            if ragged:
                st["off"] = (np.arange(rows) % (pos + 2)).astype(np.int32)
                st["off"][rows // 2] = pos + 3
            want, info = R.select_step(st, C, N, pos, P0, N_CTX, par, None, False)
            out = run(dbg, st, C, N, pos, par, d=d)
            same(out, want, (d, C, N, ragged))
            embedding(out, info, C, N, pos, d, st["off"])
            if ragged:
                assert info["prow"][rows // 2] == 0 and len(set(info["prow"].tolist())) == pos + 2
            assert EOT in info["tok"].tolist() and len(set(info["tok"].tolist())) > 8
    # the last position of the context
    C, N, gi = 17, 7, 4
    n_prompt, par = N_CTX - gi, (N, MAX_NEW, EOT, EOT)
    st, pos = random_state(60 + d, C, N, gi, N, n_prompt=n_prompt)
    assert pos + 1 == N_CTX
    want, info = R.select_step(st, C, N, pos, n_prompt, N_CTX, par, None, True)
    out = run(dbg, st, C, N, pos, par, d=d, stop=True, n_prompt=n_prompt)
    same(out, want, (d, "pos + 1 == n_ctx"))
    embedding(out, info, C, N, pos, d)
    assert out["pos_out"] == N_CTX and np.all(out["seq"][N_CTX] >= 0) and np.all(bits(out["x_next"]) == SENT32)


# ---------------------------------------------------------------- 6. a whole search, step by step
@pytest.mark.parametrize("seed,C,N,max_cand", R.SEARCHES)
def test_a_whole_search_step_by_step(dbg, seed, C, N, max_cand):
    """The hook, then wmdbg_beam_reorder on a cache of L2 = 1, H = 1, T = n_ctx, for max_new steps over the scripts whose
    branches tests/test_beam_step_cpu.py counts: after every launch the whole state equals the restatement's (which then carries
    the search), at the end the windows' hypotheses are BeamWindowNp's.  Rules and early stop on; ancestry for N = 3."""
    rows, anc = C * N, N == 3
    par = (max_cand, MAX_NEW, EOT, EOT)
    g = np.random.default_rng(seed)
    cache = g.integers(0, 65536, size=(1, rows, 1, N_CTX, 64), dtype=np.uint16)
    last = None
    for gi, st, sel, info, re in R.search(seed, C, N, max_cand, anc=anc):
        pos = P0 - 1 + gi
        out = run(dbg, st, C, N, pos, par, ts=TS, stop=True)
        same(out, sel, (seed, gi, "select"))
        assert out["pos_out"] == pos + 1
        assert np.array_equal(bits(out["x_next"][:rows]), bits(R.embed_x(world(64).emb, world(64).pemb, info["tok"], info["prow"])))
        # the re-parenting launch behind it, in place on the hook's buffers
        lp = np.concatenate([out["logprob"], R.sent_f32((N_CTX - MAX_NEW, rows))])
        seq = np.ascontiguousarray(out["seq"][:N_CTX])
        want_c = cache.copy()
        for w in range(C):
            for k in range(N):
                if not out["wdone"][w]:
                    want_c[:, w * N + k, :, :pos + 1] = cache[:, w * N + int(out["src"][w * N + k]), :, :pos + 1]
        src, wdone = np.ascontiguousarray(out["src"][:rows]), np.ascontiguousarray(out["wdone"][:C])
        rc = dbg.lib.wmdbg_beam_reorder(dbg.handle, cache.ctypes.data_as(vp), 1, rows, 1, N_CTX, N, pos, P0, src.ctypes.data_as(vp),
                                        wdone.ctypes.data_as(vp), seq.ctypes.data_as(vp), lp.ctypes.data_as(vp))
        assert rc == 0, dbg.lib.wm_last_error()
        assert np.array_equal(cache, want_c), (seed, gi)
        assert np.array_equal(seq, re["seq"][:N_CTX]) and np.array_equal(bits(lp[:MAX_NEW]), bits(re["logprob"])), (seed, gi, "reorder")
        assert np.all(bits(lp[MAX_NEW:]) == SENT32)
        last = re
    script, budget = R.search_script(seed, C, N, MAX_NEW, N_TEXT, EOT)
    same_hypotheses(last, drive_windows(script, budget, C, N, max_cand, EOT), C, N, P0)


# ---------------------------------------------------------------- 7. rejections
def test_rejections_launch_nothing(dbg):
    """Every geometry with which the kernel could leave a buffer: WM_ERR_INVALID, a message that names the hook, and every buffer
    still holds what it held."""
    C, N, gi, max_cand = 5, 3, 2, 4
    base, pos = random_state(1, C, N, gi, max_cand, ts=TS)
    base["off"] = np.zeros(C * N, np.int32)
    par = (max_cand, MAX_NEW, EOT, EOT)
    big, _ = random_state(2, 17, 8, gi, max_cand)

    def edit(key, index, value):
        st = R.copy_state(base)
        st[key][index] = value
        return st
    cases = [("C < 1", base, dict(C=0)), ("N < 1", base, dict(N=0)), ("N > 8", base, dict(N=9)), ("cap < C", base, dict(cap=C - 1)),
             ("rows > 128", big, dict(C=17, N=8)),
             ("pos < n_prompt - 1", base, dict(pos=P0 - 2)), ("pos >= n_ctx", base, dict(pos=N_CTX, par=(max_cand, 64, EOT, EOT))),
             ("gi >= max_new", base, dict(par=(max_cand, gi, EOT, EOT))),
             ("max_cand < 1", base, dict(par=(0, MAX_NEW, EOT, EOT))), ("max_cand > 16", base, dict(par=(17, MAX_NEW, EOT, EOT))),
             ("fin_n > max_cand", edit("fin_n", C - 1, max_cand + 1), {}), ("fin_n < 0", edit("fin_n", 0, -1), {}),
             ("list_n < 0", edit("list_n", 4, -1), {}), ("list_n > N + 1", edit("list_n", C * N - 1, N + 2), {}),
             ("a token at n_vocab", edit("list_tok", (0, 0), V), {}), ("a negative token", edit("list_tok", (0, 0), -1), {}),
             ("pad outside the vocabulary", base, dict(par=(max_cand, MAX_NEW, EOT, V))),
             ("a negative off", edit("off", 3, -1), {}),
             ("d 80", base, dict(d=80)), ("d 0", base, dict(d=0)), ("d 1344", base, dict(d=1344))]
    for what, st, kw in cases:
        if what.startswith("a") and "token" in what:
            st["list_n"][0] = max(1, int(st["list_n"][0]))        # (the entry is inside the list)
        a = dict(C=C, N=N, pos=pos, par=par, d=64, cap=None)
        a.update(kw)
        out = run(dbg, st, a["C"], a["N"], a["pos"], a["par"], d=a["d"], ts=TS, stop=True, cap=a["cap"], expect_ok=False)
        assert out["rc"] == WM_ERR_INVALID, what
        assert b"wmdbg_beam_step" in dbg.lib.wm_last_error(), (what, dbg.lib.wm_last_error())
        same(out, st, what)
        for k in ("x_next", "xb_next", "stats_next", "mean_next"):
            assert np.all(out[k] == HOST_FILL), (what, k)
        assert out["pos_out"] == SENT and out["tail"] == SENT, what
    # and the state the cases were cut from is accepted
    out = run(dbg, base, C, N, pos, par, ts=TS, stop=True)
    same(out, R.select_step(base, C, N, pos, P0, N_CTX, par, TS, True)[0], "accepted")
