"""One close of a beam group (csrc/beam.hip beam_select_kernel, then beam_reorder_kernel's history half) restated in plain
Python over lists and numpy arrays: no device code, no wm_beam_select.  The tests compare the kernel's buffers with these
bit for bit (tests/test_beam_step_kernel_gpu.py), after tests/test_beam_step_cpu.py has held multi-step searches through
select_step + reorder to BeamWindowNp of tests/test_beam_cpu.py.

A state is a dict of numpy arrays in the device's shapes (rows = C * N; per-window arrays have cap >= C entries, per-row arrays
cap * N; what lies behind the group's is never touched):
  budget, wdone, wsteps, fin_n i32 [cap];  sum f32, list_n, src, done, live_rows i32 [cap * N];  list_tok i32 / list_lp f32
  [cap * N][9];  fin_len i32 / fin_sum f32 / fin_src i32 [cap][16];  fin_tok i32 / fin_lp f32 [cap][16][n_ctx];  anc i32
  [max_new][rows] or None;  seq i32 [n_ctx + 1][rows];  logprob f32 [max_new][rows];  hist, rng i32 [cap * N][4];  n_live i32 [1].

The contract of one step at position pos (generated index gi = pos + 1 - n_prompt), per window w < C with rows w * N + k:
  * wdone[w] != 0 (the window has left): every row takes `pad` with log-prob 0, src = anc[gi] = the slot itself, done = 1;
    sum, fin_*, wsteps, hist and rng stay.
  * else the selection rule (beam_select_np) over the window's sums and lists, beam 0 alone at gi == 0, room = max_cand -
    fin_n[w].  Kept finished hypothesis f goes to slot fin_n[w] + f: fin_tok / fin_lp = the SOURCE beam's seq / logprob history
    (generated indices 0 .. gi - 1) followed by (eot, its log-prob), fin_len = gi + 1, fin_sum, and -- in an aligned group (anc
    given) -- fin_src.  Slot k takes token, log-prob, sum and src of the rule; anc[gi] = src; with the timestamp rules its
    (hist, rng) = ts_advance(hist[src], token).  fin_n += kept; the window leaves when fin_n >= max_cand or gi + 1 >=
    budget[w]: wdone = leaves, wsteps = gi + 1; done = leaves or the beam is dead (sum == -inf).
  * early stop on: done [rows] as above, live_rows = the ascending compact list of the rows that are not done, n_live its
    length; entries behind it stay.
  * seq[pos + 1] and logprob[gi] take the rows' tokens and log-probs; the position becomes pos + 1; when pos + 1 < n_ctx every
    row's token is embedded at positional row pos + 1 (a ragged group: max(pos + 1 - off[row], 0))."""
import numpy as np

from spec_ref import ts_advance, ts_start

MAXN, LIST, HYPS = 8, 9, 16          # WM_MAX_BEAM, WM_MAX_BEAM + 1, WM_MAX_BEAM_HYPS
f32 = np.float32
NINF = f32(-np.inf)


def beam_select_np(N, n_from, eot, pad, room, sums, lists):
    """lists[j] = [(token, lp)], best first.  Returns (n_next, src, tok, lp, new_sum, fins) with fins = [(src, lp, sum)]."""
    cands = []
    for j in range(n_from):
        if sums[j] == NINF:
            continue
        for e, (t, lp) in enumerate(lists[j]):
            cands.append((f32(f32(sums[j]) + f32(lp)), j, e, int(t), f32(lp)))
    cands.sort(key=lambda c: -float(c[0]))          # Python's sort is stable: ties keep (beam, entry) order
    src, tok, lps, new, fins = [], [], [], [], []
    for score, j, _, t, lp in cands:
        if len(src) == N:
            break
        if eot >= 0 and t == eot:
            if len(fins) < room:
                fins.append((j, lp, score))
        else:
            src.append(j); tok.append(t); lps.append(lp); new.append(score)
    n_next = len(src)
    for k in range(n_next, N):
        src.append(k); tok.append(pad); lps.append(f32(0)); new.append(NINF)
    return n_next, src, tok, lps, new, fins


def copy_state(st):
    return {k: (None if v is None else np.array(v, copy=True)) for k, v in st.items()}


def window_lists(st, row0, N):
    """the lists of a window's beams as beam_select_np takes them"""
    return [[(int(st["list_tok"][row0 + j, e]), f32(st["list_lp"][row0 + j, e])) for e in range(int(st["list_n"][row0 + j]))]
            for j in range(N)]


def select_step(st, C, N, pos, n_prompt, n_ctx, par, ts=None, stop=False):
    """One step of the contract above.  par = (max_cand, max_new, eot, pad); ts = (ts_begin, eot, n_vocab, max_initial) or None.
    Returns (state behind the step -- new arrays, st is not modified --, info) with info = dict(pos = pos + 1, tok = the token
    each row took [rows], embedded = whether the rows were embedded, prow = their positional rows, events = per window the set
    of branches it took)."""
    max_cand, max_new, eot, pad = par
    gi, rows = pos + 1 - n_prompt, C * N
    assert 0 <= gi < max_new and pos + 1 <= n_ctx
    out = copy_state(st)
    done = np.zeros(rows, np.int32)
    tok_of = np.zeros(rows, np.int64)
    events = [set() for _ in range(C)]
    for w in range(C):
        row0 = w * N
        r = slice(row0, row0 + N)
        if st["wdone"][w] != 0:
            events[w].add("was_done")
            out["seq"][pos + 1, r] = pad
            out["logprob"][gi, r] = f32(0)
            out["src"][r] = np.arange(N)
            if st["anc"] is not None:
                out["anc"][gi, r] = np.arange(N)
            done[r] = 1
            tok_of[r] = pad
            continue
        fin0 = int(st["fin_n"][w])
        sums = [f32(v) for v in st["sum"][r]]
        lists = window_lists(st, row0, N)
        n_from = 1 if gi == 0 else N
        n_next, src, tok, lp, new, fins = beam_select_np(N, n_from, eot, pad, max_cand - fin0, sums, lists)
        for f, (j, flp, fsum) in enumerate(fins):
            slot = fin0 + f
            out["fin_tok"][w, slot, :gi] = st["seq"][n_prompt:n_prompt + gi, row0 + j]
            out["fin_lp"][w, slot, :gi] = st["logprob"][:gi, row0 + j]
            out["fin_tok"][w, slot, gi] = eot
            out["fin_lp"][w, slot, gi] = flp
            out["fin_len"][w, slot] = gi + 1
            out["fin_sum"][w, slot] = fsum
            if st["anc"] is not None:
                out["fin_src"][w, slot] = j
        nfin = fin0 + len(fins)
        leaves = nfin >= max_cand or gi + 1 >= int(st["budget"][w])
        for k in range(N):
            row = row0 + k
            out["seq"][pos + 1, row] = tok[k]
            out["logprob"][gi, row] = lp[k]
            out["sum"][row] = new[k]
            out["src"][row] = src[k]
            if st["anc"] is not None:
                out["anc"][gi, row] = src[k]
            if ts is not None:      # the state follows the source beam, not the slot
                h, g = ts_advance(tuple(int(v) for v in st["hist"][row0 + src[k]]), tok[k], ts[0], ts[1], ts[2])
                out["hist"][row], out["rng"][row] = h, g
            done[row] = 1 if (leaves or new[k] == NINF) else 0
            tok_of[row] = tok[k]
        out["fin_n"][w] = nfin
        out["wdone"][w] = 1 if leaves else 0
        out["wsteps"][w] = gi + 1
        # the branches this window took (conditions on the inputs: tests/test_beam_step_cpu.py asserts the scripts reach each)
        if src != list(range(N)):
            events[w].add("fork")
        if len(fins) >= 2:
            events[w].add("two_finish")
        if _walked_eots(N, n_from, eot, sums, lists) > len(fins):
            events[w].add("eot_dropped")
        if n_next < N:
            events[w].add("dead_beam")
        if nfin >= max_cand:
            events[w].add("leaves_by_max_cand")
        elif leaves:
            events[w].add("leaves_by_budget")
        if gi == max_new - 1:
            events[w].add("live_at_the_last_step")
        if ts is not None and any(st["hist"][row0 + src[k]].tolist() != st["hist"][row0 + k].tolist() for k in range(n_next)):
            events[w].add("rule_state_moves")       # a slot inherits a rule state other than the one it held
    if stop:
        out["done"][:rows] = done
        live = np.flatnonzero(done == 0)
        out["live_rows"][:live.size] = live
        out["n_live"][0] = live.size
    embedded = pos + 1 < n_ctx
    prow = np.full(rows, pos + 1) if st.get("off") is None else np.maximum(pos + 1 - np.asarray(st["off"], np.int64), 0)
    return out, dict(pos=pos + 1, tok=tok_of, embedded=embedded, prow=prow, events=events)


def _walked_eots(N, n_from, eot, sums, lists):
    """eot candidates the walk meets before it stops (the kept ones and the ones dropped for want of room)"""
    if eot < 0:
        return 0
    return len(beam_select_np(N, n_from, eot, 0, 1 << 30, sums, lists)[5])


def reorder(st, C, N, pos, n_prompt):
    """beam_reorder_kernel restricted to the histories, behind the close of position pos: generated indices 0 .. gi - 1 of
    every window's rows are gathered by src (index gi, the new token, is in the new order already)."""
    gi = pos + 1 - n_prompt
    out = copy_state(st)
    for w in range(C):
        for k in range(N):
            a, b = w * N + k, w * N + int(st["src"][w * N + k])
            out["seq"][n_prompt:n_prompt + gi, a] = st["seq"][n_prompt:n_prompt + gi, b]
            out["logprob"][:gi, a] = st["logprob"][:gi, b]
    return out


def embed_x(emb, pemb, tok, prow):
    """check_embedding's rule for the f32 row: f32(bf16 emb[token]) + pemb[positional row], one f32 add"""
    return (np.asarray(emb, f32)[np.asarray(tok)] + np.asarray(pemb, f32)[np.asarray(prow)]).astype(f32)


def hypotheses(st, w, N, n_prompt):
    """Window w's hypotheses in output order, as BeamWindowNp.hypotheses gives them: the finished ones as they finished, then
    the live beams by descending sum (stable) until there are N: [(tokens, log-prob bits, sum bits)]."""
    hyps = []
    for s in range(int(st["fin_n"][w])):
        n = int(st["fin_len"][w, s])
        hyps.append((st["fin_tok"][w, s, :n].tolist(), st["fin_lp"][w, s, :n].view(np.uint32).tolist(),
                     int(st["fin_sum"][w, s:s + 1].view(np.uint32)[0])))
    sums = st["sum"][w * N:(w + 1) * N]
    n = int(st["wsteps"][w])
    for j in sorted((j for j in range(N) if sums[j] != NINF), key=lambda j: -float(sums[j])):
        if len(hyps) >= N:
            break
        hyps.append((st["seq"][n_prompt:n_prompt + n, w * N + j].tolist(), st["logprob"][:n, w * N + j].view(np.uint32).tolist(),
                     int(sums[j:j + 1].view(np.uint32)[0])))
    return hyps


# ---------------------------------------------------------------- scripted searches (the CPU and the GPU tests share the seeds)
SENT = -7777                         # ints nothing may write
SENT_F32 = 0x7fc0dead                # WMDBG_SENTINEL_F32


def sent_f32(shape):
    return np.full(shape, SENT_F32, np.uint32).view(f32)


def fresh(C, N, cap, n_ctx, max_new, anc=True):
    """a state nobody has written: every array at its sentinel (the token buffer a different negative value per cell)"""
    rows, nr = C * N, cap * N
    st = {k: np.full(cap, SENT, np.int32) for k in ("budget", "wdone", "wsteps", "fin_n")}
    st.update({k: np.full(nr, SENT, np.int32) for k in ("list_n", "src", "done")})
    st.update(sum=sent_f32(nr), live_rows=np.full(nr, -1, np.int32), n_live=np.full(1, SENT, np.int32),
              list_tok=np.full((nr, LIST), SENT, np.int32), list_lp=sent_f32((nr, LIST)),
              fin_len=np.full((cap, HYPS), SENT, np.int32), fin_sum=sent_f32((cap, HYPS)), fin_src=np.full((cap, HYPS), SENT, np.int32),
              fin_tok=np.full((cap, HYPS, n_ctx), SENT, np.int32), fin_lp=sent_f32((cap, HYPS, n_ctx)),
              anc=np.full((max_new, rows), SENT, np.int32) if anc else None,
              seq=-(1000 + np.arange((n_ctx + 1) * rows, dtype=np.int32)).reshape(n_ctx + 1, rows),
              logprob=sent_f32((max_new, rows)), hist=np.full((nr, 4), SENT, np.int32), rng=np.full((nr, 4), SENT, np.int32), off=None)
    return st


def put_lists(st, row0, lists):
    """the lists of a window's beams into the state: entries behind a list keep what they held"""
    for j, l in enumerate(lists):
        st["list_n"][row0 + j] = len(l)
        for e, (t, p) in enumerate(l):
            st["list_tok"][row0 + j, e] = t
            st["list_lp"][row0 + j, e] = p


def random_lists(rng, N, pool, eot, p_eot, p_short, quantum=0.0):
    """N lists of up to N + 1 distinct tokens of `pool` (a count: the ids below it; or the ids themselves, eot not among them)
    with descending log-probs; with probability p_eot a list holds eot, with probability p_short it has 0 .. N entries.
    quantum: log-probs on a coarse grid (exact score ties)."""
    lists = []
    for _ in range(N):
        n = N + 1
        if rng.random() < p_short:
            n = int(rng.integers(0, N + 1))
        toks = [int(t) for t in rng.choice(pool, size=n, replace=False)]
        if toks and eot >= 0 and rng.random() < p_eot:
            toks[int(rng.integers(0, len(toks)))] = eot
        lp = -rng.exponential(2.0, size=len(toks))
        if quantum:
            lp = np.round(lp / quantum) * quantum
        lp = np.sort(lp.astype(f32))[::-1]
        lists.append([(t, f32(v)) for t, v in zip(toks, lp)])
    return lists


def search_script(seed, C, N, max_new, n_text, eot):
    """The lists of a whole search, script[gi][w] = the N lists of window w at generated index gi, and the windows' budgets.
    Random lists with eot at a fixed probability; the rare branches are planted by hand: windows 1 and 2 see every beam's list
    empty at gi = 2 (dead beams, then an empty window), windows 3 and 4 get eot on top of two beams' lists at gi = 1 (two
    finish in one step), windows 0 and 5 never see eot and keep the whole budget (live at the last step)."""
    rng = np.random.default_rng(seed)
    pool = np.array([t for t in range(n_text) if t != eot] + list(range(TS[0], N_VOCAB)))   # text and timestamps: the beams' rule states differ
    script = [[random_lists(rng, N, pool, eot, 0.3, 0.25, 0.5 if (gi + w) % 3 == 0 else 0.0) for w in range(C)] for gi in range(max_new)]
    budget = np.array([(max_new, 1, 2, max_new // 2, max_new - 1, max_new)[w % 6] if w >= 6 else max_new for w in range(C)], np.int32)
    other = [t for t in range(n_text)]
    for gi in range(max_new):
        for w in (0, 5):
            if w < C:
                script[gi][w] = [[((other[(3 * e + 7 * j + gi) % n_text]) if t == eot else t, p) for e, (t, p) in enumerate(l)]
                                 for j, l in enumerate(script[gi][w])]
                script[gi][w] = [_distinct(l, n_text, eot) for l in script[gi][w]]
                if gi == 0 and not script[gi][w][0]:
                    script[gi][w][0] = [(1 + w, f32(-0.5)), (9 + w, f32(-1.5))]
    if max_new > 2:
        for w in (1, 2):
            if w < C:
                script[2][w] = [[] for _ in range(N)]
    if max_new > 1 and N >= 2:
        for w in (3, 4):
            if w < C:
                for gi in (0, 1):       # no eot and full lists in front, so that two beams are alive at gi = 1
                    script[gi][w] = [_distinct([(other[(5 * e + 11 * j + gi + w) % n_text], f32(-0.25 * (e + 1))) for e in range(N + 1)],
                                               n_text, eot) for j in range(N)]
                for j in (0, 1):
                    script[1][w][j] = [(eot, f32(-0.125))] + script[1][w][j][1:]
    return script, budget


def _distinct(l, n_text, eot):
    """a list's tokens made distinct (the list kernel never lists an id twice), none of them eot"""
    seen, out = set(), []
    for t, p in l:
        while t in seen or t == eot:
            t = (t + 1) % n_text
        seen.add(t)
        out.append((t, p))
    return out


def search_start(C, N, cap, n_ctx, n_prompt, max_new, budget, anc, ts=None):
    """the state wm_model_beam_begin leaves in front of generated index 0: sums, sources, flags and counts zero, the prompt in
    the token buffer, the timestamp rules' initial state; everything else at its sentinel"""
    rows = C * N
    st = fresh(C, N, cap, n_ctx, max_new, anc)
    st["budget"][:C] = budget
    for k in ("wdone", "wsteps", "fin_n"):
        st[k][:C] = 0
    st["sum"][:rows] = 0
    st["src"][:rows] = 0
    st["done"][:rows] = 0
    st["seq"][:n_prompt] = 50 + np.arange(n_prompt)[:, None]
    if ts is not None:
        h, g = ts_start(ts[0], ts[2], ts[3])
        st["hist"][:rows], st["rng"][:rows] = h, g
    return st


def load_lists(st, script_gi, C, N):
    """a step's lists into the state, as the list kernel would leave them: rows of windows that have left and dead beams get
    list_n = 0 and keep their old entries"""
    for w in range(C):
        for j in range(N):
            row = w * N + j
            if st["wdone"][w] != 0 or st["sum"][row] == NINF:
                st["list_n"][row] = 0
            else:
                put_lists(st, row, [script_gi[w][j]])


# the whole searches of the GPU test (seed, C, N, max_cand), and their geometry
N_CTX, N_PROMPT, N_VOCAB, MAX_NEW, EOT, N_TEXT = 24, 3, 96, 16, 70, 70
TS = (80, EOT, N_VOCAB, 5)           # ts_begin, eot, n_vocab, max_initial
SEARCHES = [(101, 33, 3, 1), (102, 33, 3, 3), (103, 33, 3, 16), (104, 17, 7, 1), (105, 17, 7, 7), (106, 17, 7, 16)]
BRANCHES = ("fork", "two_finish", "eot_dropped", "dead_beam", "leaves_by_max_cand", "leaves_by_budget", "was_done",
            "live_at_the_last_step", "rule_state_moves")


def search(seed, C, N, max_cand, anc=True, ts=TS, stop=True):
    """A whole scripted search through select_step + reorder.  Yields per generated index (gi, the state in front of the step
    with its lists loaded, the state behind select_step, its info, the state behind reorder)."""
    script, budget = search_script(seed, C, N, MAX_NEW, N_TEXT, EOT)
    par = (max_cand, MAX_NEW, EOT, EOT)
    st = search_start(C, N, C + 2, N_CTX, N_PROMPT, MAX_NEW, budget, anc, ts)
    for gi in range(MAX_NEW):
        pos = N_PROMPT - 1 + gi
        load_lists(st, script[gi], C, N)
        sel, info = select_step(st, C, N, pos, N_PROMPT, N_CTX, par, ts, stop)
        re = reorder(sel, C, N, pos, N_PROMPT)
        yield gi, st, sel, info, re
        st = re
