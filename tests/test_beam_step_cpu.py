"""CPU tests of the restatement the select kernel is held to (tests/beam_step_ref.py select_step + reorder, which
tests/test_beam_step_kernel_gpu.py compares with beam_select_kernel bit for bit): it is not trusted alone.  Multi-step searches
of scripted lists through it give, per window, what BeamWindowNp of tests/test_beam_cpu.py gives; the scripts of the GPU test --
its exact seeds and shapes -- reach every branch of the kernel; the ctypes mirror of struct wmdbg_beam_io agrees with the
header."""
import ctypes

import numpy as np
import pytest

import beam_step_ref as R
from test_beam_cpu import BeamWindowNp

f32 = np.float32
vp, i32 = ctypes.c_void_p, ctypes.c_int32


class BeamIo(ctypes.Structure):
    """struct wmdbg_beam_io"""
    _fields_ = [(n, i32) for n in ("C", "N", "cap", "n_ctx", "pos", "n_prompt", "d", "n_vocab", "max_cand", "max_new", "eot", "pad",
                                   "ts_on")] + \
               [("ts_par", i32 * 4), ("stop_on", i32)] + \
               [(n, vp) for n in ("budget", "sum", "list_n", "list_tok", "list_lp", "src", "wdone", "wsteps", "fin_n", "fin_len", "fin_sum",
                                  "fin_src", "fin_tok", "fin_lp", "anc", "seq", "logprob", "hist", "rng", "done", "live_rows", "n_live",
                                  "off", "emb", "pemb", "x_next", "xb_next", "stats_next", "mean_next")] + \
               [("stats_tail_nonzero", i32), ("pos_out", i32)]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def drive_windows(script, budget, C, N, max_cand, eot):
    """BeamWindowNp per window over the same script: a window is stepped while it has not left"""
    wins = [BeamWindowNp(N, max_cand, eot, int(budget[w])) for w in range(C)]
    for gi in range(len(script)):
        for w, win in enumerate(wins):
            if not win.done:
                win.step(script[gi][w])
    return wins


def same_hypotheses(st, wins, C, N, n_prompt):
    for w, win in enumerate(wins):
        got = R.hypotheses(st, w, N, n_prompt)
        want = [(list(t), bits(np.array(l, f32)).tolist(), int(bits(np.array([s], f32))[0])) for t, l, s in win.hypotheses()]
        assert got == want, (w, got, want)
        assert int(st["wsteps"][w]) == win.gi and int(st["fin_n"][w]) == len(win.finished) and bool(st["wdone"][w]) == win.done


@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
def test_searches_through_the_restatement_give_what_BeamWindowNp_gives(N):
    """48 windows per beam width (240 in all) x 10 steps, random scripts with eot, short lists and score ties, per-window
    budgets, max_cand below, equal to and above N; rules, early stop and ancestry on or off by the case."""
    n_ctx, n_prompt, max_new, n_text, eot = 20, 2, 10, 14, 14
    for case, (C, max_cand) in enumerate(((16, max(1, N - 1)), (16, N), (16, min(R.HYPS, N + 3)))):
        rng = np.random.default_rng(1000 * N + case)
        script = [[R.random_lists(rng, N, n_text, eot, 0.35, 0.3, 0.5 if (gi + w) % 2 else 0.0) for w in range(C)] for gi in range(max_new)]
        budget = rng.integers(1, max_new + 1, size=C).astype(np.int32)
        ts = (16, eot, 24, 3) if case != 1 else None
        st = R.search_start(C, N, C + 1, n_ctx, n_prompt, max_new, budget, case != 2, ts)
        for gi in range(max_new):
            pos = n_prompt - 1 + gi
            R.load_lists(st, script[gi], C, N)
            sel, info = R.select_step(st, C, N, pos, n_prompt, n_ctx, (max_cand, max_new, eot, eot), ts, case == 0)
            assert info["pos"] == pos + 1
            st = R.reorder(sel, C, N, pos, n_prompt)
            # what lies behind the group's stays what it was
            for k in ("wdone", "wsteps", "fin_n", "fin_len", "fin_tok"):
                assert np.all(st[k][C:] == R.SENT), k
            assert np.all(st["src"][C * N:] == R.SENT) and np.all(bits(st["sum"][C * N:]) == R.SENT_F32)
        same_hypotheses(st, drive_windows(script, budget, C, N, max_cand, eot), C, N, n_prompt)


def test_a_hand_made_window():
    """test_beam_cpu's whole window (2 finished of 3 wanted at the budget, N = 4) through the restatement, field by field"""
    N, n_ctx, n_prompt, max_new, E = 4, 8, 2, 4, 9
    st = R.search_start(1, N, 1, n_ctx, n_prompt, max_new, [2], True, None)
    steps = [[[(1, f32(-1)), (9, f32(-1.5)), (2, f32(-2)), (3, f32(-3)), (4, f32(-4))]] * 4,
             [[(9, f32(-0.1)), (5, f32(-0.2))], [(6, f32(-0.1))], [(7, f32(-9))], []]]
    R.load_lists(st, [steps[0]], 1, N)
    st, info = R.select_step(st, 1, N, 1, n_prompt, n_ctx, (3, max_new, E, E), None, True)
    assert st["seq"][2].tolist() == [1, 2, 3, 4] and st["src"][:4].tolist() == [0, 0, 0, 0] and st["anc"][0].tolist() == [0] * 4
    assert (int(st["fin_n"][0]), int(st["wdone"][0]), int(st["wsteps"][0])) == (1, 0, 1) and st["fin_tok"][0, 0, :1].tolist() == [9]
    assert st["done"][:4].tolist() == [0] * 4 and st["live_rows"][:4].tolist() == [0, 1, 2, 3] and int(st["n_live"][0]) == 4
    assert info["events"][0] == {"fork"}
    st = R.reorder(st, 1, N, 1, n_prompt)
    R.load_lists(st, [steps[1]], 1, N)
    st, info = R.select_step(st, 1, N, 2, n_prompt, n_ctx, (3, max_new, E, E), None, True)
    assert st["seq"][3].tolist() == [5, 6, 7, E] and st["src"][:4].tolist() == [0, 1, 2, 3]
    assert bits(st["sum"][:4]).tolist() == bits(np.array([f32(-1) + f32(-0.2), f32(-2) + f32(-0.1), f32(-3) + f32(-9), -np.inf], f32)).tolist()
    assert (int(st["fin_n"][0]), int(st["wdone"][0]), int(st["wsteps"][0])) == (2, 1, 2)
    assert st["fin_tok"][0, 1, :2].tolist() == [1, 9] and int(st["fin_len"][0, 1]) == 2 and int(st["fin_src"][0, 1]) == 0
    assert st["done"][:4].tolist() == [1] * 4 and int(st["n_live"][0]) == 0 and st["live_rows"][:4].tolist() == [0, 1, 2, 3]   # (the old list stays)
    assert info["events"][0] == {"dead_beam", "leaves_by_budget"}
    assert [h[0] for h in R.hypotheses(st, 0, N, n_prompt)] == [[9], [1, 9], [1, 5], [2, 6]]
    # the window has left: padding, and nothing else moves
    before = R.copy_state(st)
    st, info = R.select_step(st, 1, N, 3, n_prompt, n_ctx, (3, max_new, E, E), None, True)
    assert info["events"][0] == {"was_done"} and st["seq"][4].tolist() == [E] * 4 and bits(st["logprob"][2]).tolist() == [0] * 4
    for k in ("sum", "fin_n", "fin_len", "fin_sum", "fin_tok", "fin_lp", "fin_src", "wsteps", "wdone"):
        assert np.array_equal(bits(st[k]) if st[k].dtype == f32 else st[k], bits(before[k]) if st[k].dtype == f32 else before[k]), k


def test_the_scripts_of_the_gpu_test_reach_every_branch():
    """The whole searches of tests/test_beam_step_kernel_gpu.py, on the restatement's own run: every branch of the kernel is
    taken in at least two windows, and the searches give what BeamWindowNp gives."""
    seen = {b: set() for b in R.BRANCHES}
    for seed, C, N, max_cand in R.SEARCHES:
        last = None
        for gi, st, sel, info, re in R.search(seed, C, N, max_cand):
            for w, ev in enumerate(info["events"]):
                assert ev <= set(R.BRANCHES)
                for b in ev:
                    seen[b].add((seed, w))
            last = re
        script, budget = R.search_script(seed, C, N, R.MAX_NEW, R.N_TEXT, R.EOT)
        same_hypotheses(last, drive_windows(script, budget, C, N, max_cand, R.EOT), C, N, R.N_PROMPT)
    counts = {b: len(v) for b, v in seen.items()}
    assert all(n >= 2 for n in counts.values()), counts
    # and within each geometry alone
    for geom in ((33, 3), (17, 7)):
        seeds = {s for s, C, N, _ in R.SEARCHES if (C, N) == geom}
        per = {b: len({x for x in v if x[0] in seeds}) for b, v in seen.items()}
        assert all(n >= 2 for n in per.values()), (geom, per)


def test_layout_of_the_hook_struct(pkg):
    lib = pkg.binding.load_debug_library()
    lay = (i32 * 4)()
    assert lib.wmdbg_beam_step_layout(lay) == 0
    assert list(lay) == [ctypes.sizeof(BeamIo), BeamIo.ts_par.offset, BeamIo.budget.offset, BeamIo.x_next.offset], list(lay)
    assert lib.wmdbg_beam_step_layout(None) != 0
    assert not hasattr(pkg.binding.load_library(), "wmdbg_beam_step")
