"""Given panels (wm_set_given_panel) restated over plain lists -- tests/test_given_panel_cpu.py,
tests/test_given_panel_kernel_gpu.py and tests/test_given_panel_gpu.py read this one file.

  plan(...)        -- tx_plan.cpp wm_given_panel_plan: reason, w, Lp, rounds of one decode group;
  rounds_of(...)   -- the (g0, width) of the phase's rounds;
  stage_round(...) -- given_panel.hip's stage: the staged inputs and the rows' ranges;
  commit_round(...)-- its commit: kept tokens, pads, log-probs, done, the live list, the committed rule state.

The rule state advances by spec_ref.ts_advance (dec_close.h's, restated there); the table of a group is given_ref's."""
import numpy as np

from given_ref import group_given_np  # noqa: F401  (the group's table, as lane_prefill uploads it)
from spec_ref import DEC_MAXB, ts_advance

MAX_WIDTH = 8
# the reasons a group is not served, in the order the rule tests
SERVED, WIDTH1, NO_TABLE, CANDIDATES, RAGGED, NO_X, SAMP_ROWS, TRUNC, ALT, SB_TABLES, SB, CST, REP, ACAP, F32, NARROW, NO_PHASE = range(17)
# the group's mode as a bit word
B_GIVEN, B_CAND, B_OFF, B_X, B_SROWS, B_TRUNC, B_ALT, B_SBT, B_SB, B_CST, B_REP, B_ACAP, B_F32, B_SAMPLE = (1 << i for i in range(14))
_ORDER = ((B_CAND, CANDIDATES), (B_OFF, RAGGED), (None, NO_X), (B_SROWS, SAMP_ROWS), (B_TRUNC | B_SAMPLE, TRUNC), (B_ALT, ALT),
          (B_SBT, SB_TABLES), (B_SB, SB), (B_CST, CST), (B_REP, REP), (B_ACAP, ACAP), (B_F32, F32))


def plan(G, width, lens, budgets, max_new, P, n_text_ctx, bits):
    """(reason, w, Lp, rounds).  lens [G]; budgets [G] or None.  Lp: the largest L <= max_new with P + L - 1 < n_text_ctx such
    that every row is given or finished at every index of [1, L)."""
    if width <= 1:
        return (WIDTH1, 0, 0, 0)
    if not bits & B_GIVEN:
        return (NO_TABLE, 0, 0, 0)
    for bit, reason in _ORDER:
        if (not bits & B_X) if bit is None else (bits & bit):
            return (reason, 0, 0, 0)
    w = min(width, MAX_WIDTH, DEC_MAXB // G)
    if w < 2:
        return (NARROW, w, 0, 0)
    L = 0
    for cand in range(1, min(max_new, n_text_ctx - P) + 1):   # the definition, not the closed form
        ok = True
        for r in range(G):
            fin = min(budgets[r], max_new) if budgets is not None else max_new
            ok = ok and all(gi < lens[r] or gi >= fin for gi in range(1, cand))
        if ok:
            L = cand
    if L <= 1:
        return (NO_PHASE, w, L, 0)
    return (SERVED, w, L, -(-(L - 1) // w))


def rounds_of(w, Lp):
    """[(g0, width)] of the phase over generated indices [1, Lp)"""
    return [(g0, min(w, Lp - g0)) for g0 in range(1, Lp, w)]


def stage_round(st, G, w, g0, P, n_ctx, ts, pad_tok, first):
    """st: dict(seq [n_ctx][G], lens [G], tok [G][stride], hist [G][4], rng [G][4] -- the step path's -- and, behind the first
    round, chist / crng [G][4]).  Writes the inputs of rows s >= 1 at positions pos + s and returns the rows' ranges [G * w][4]
    (None without rules).  ts = (ts_begin, eot, n_vocab) or None."""
    pos = P + g0 - 1
    if ts is not None and first:
        st["chist"] = [list(h) for h in st["hist"][:G]]
        st["crng"] = [list(r) for r in st["rng"][:G]]
    rows = [None] * (G * w) if ts is not None else None
    for c in range(G):
        hist = list(st["chist"][c]) if ts is not None else None
        if ts is not None:
            rows[c * w] = list(st["crng"][c])
        for s in range(1, w):
            p = pos + s
            if p >= n_ctx:
                break
            gi = g0 + s - 1
            tok = st["tok"][c][gi] if gi < len(st["tok"][c]) and gi < st["lens"][c] else pad_tok
            st["seq"][p][c] = tok
            if ts is not None:
                hist, r = ts_advance(hist, tok, ts[0], ts[1], ts[2])
                rows[c * w + s] = list(r)
    return rows


def commit_round(st, G, w, g0, P, max_new, wtok, wlp, eot, budgets, pad_tok, ts, last):
    """wtok / wlp [G * w]: what the close left for every row.  st additionally holds done [G] and logprob [max_new][G].  A live
    window keeps its tokens up to its first eot (eot >= 0) or the end of its budget, pads (pad_tok, 0.0) behind; a finished one
    pads everything.  Returns (n_live, live_rows); st["pos"] = the position after the round; behind the last round st["hist"] /
    st["rng"] hold the committed state in the step path's layout."""
    pos = P + g0 - 1
    for c in range(G):
        live = not st["done"][c]
        hist = list(st["chist"][c]) if ts is not None else None
        rng = list(st["crng"][c]) if ts is not None else None
        for i in range(w):
            gi = g0 + i
            tok, lp = pad_tok, 0.0
            if live:
                tok, lp = wtok[c * w + i], wlp[c * w + i]
                if ts is not None:
                    hist, rng = ts_advance(hist, tok, ts[0], ts[1], ts[2])
                    rng = list(rng)
                if (eot >= 0 and tok == eot) or (budgets is not None and gi + 1 >= budgets[c]):
                    live = False
                    st["done"][c] = 1
            st["seq"][pos + 1 + i][c] = tok
            if 0 <= gi < max_new:
                st["logprob"][gi][c] = lp
        if ts is not None:
            st["chist"][c], st["crng"][c] = list(hist), list(rng)
            if last:
                st["hist"][c], st["rng"][c] = list(hist), list(rng)
    st["pos"] = pos + w
    live_rows = [c for c in range(G) if not st["done"][c]]
    return len(live_rows), live_rows


def plan_table(G, width, lens, bud, has_bud, max_new, P, n_ctx, bits):
    """plan over whole tables of cases, in numpy (the full products of the CPU test): G, width, has_bud, max_new, P, n_ctx, bits
    i32 [n]; lens, bud i32 [n][g_max] (columns >= G are not read).  Returns i32 [n][4].  Written from the definition again:
    a candidate L holds when no (row, gi) with 1 <= gi < L is neither given nor finished."""
    G, width, has_bud, max_new, P, n_ctx, bits = (np.asarray(a, np.int64) for a in (G, width, has_bud, max_new, P, n_ctx, bits))
    lens, bud = np.asarray(lens, np.int64), np.asarray(bud, np.int64)
    n, g_max = lens.shape
    out = np.zeros((n, 4), np.int64)
    reason = np.full(n, -1, np.int64)

    def first(cond, code):
        reason[(reason < 0) & cond] = code
    first(width <= 1, WIDTH1)
    first((bits & B_GIVEN) == 0, NO_TABLE)
    for bit, code in _ORDER:
        first((bits & B_X) == 0 if bit is None else (bits & bit) != 0, code)
    w = np.minimum(np.minimum(width, MAX_WIDTH), DEC_MAXB // G)
    early = reason >= 0
    first(w < 2, NARROW)
    row_on = np.arange(g_max)[None, :] < G[:, None]
    fin = np.where(has_bud[:, None] != 0, np.minimum(bud, max_new[:, None]), max_new[:, None])
    L = np.zeros(n, np.int64)
    top = np.minimum(max_new, n_ctx - P)
    for cand in range(1, int(max(top.max(), 1)) + 1):
        bad = np.zeros(n, bool)
        for gi in range(1, cand):
            bad |= (row_on & ~((gi < lens) | (gi >= fin))).any(axis=1)
        L = np.where(~bad & (cand <= top), cand, L)
    first(L <= 1, NO_PHASE)
    reason[reason < 0] = SERVED
    out[:, 0] = reason
    out[:, 1] = np.where(early, 0, w)
    out[:, 2] = np.where(early | (reason == NARROW), 0, L)
    out[:, 3] = np.where(reason == SERVED, -(-(L - 1) // np.maximum(w, 1)), 0)
    return out.astype(np.int32)
