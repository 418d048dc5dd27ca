"""A restatement of the host arithmetic of a transcribe call, written from the text of the call as it stood in
csrc/model_api.cpp before it was split into csrc/tx_plan.cpp (pure) and csrc/transcribe.cpp: how a call is cut into decode
groups and which lanes run them, the tables a group uploads, the output rows a finished group writes.
tests/test_tx_plan_cpu.py compares the hooks wmdbg_tx_plan / wmdbg_group_tables / wmdbg_group_rows_out with it.

The plan is vectorised over numpy arrays of cases (every argument broadcasts); the tables and the rows are plain loops over
one case."""
import numpy as np

DEC_MAXB = 128        # WM_DEC_MAXB
GROUP_CHUNKS = 8      # kGroupChunks
XIDS_CAND = 128 + 16  # WM_XIDS_CAND
CLONES, PARTS, SOLO = 0, 1, 2


def _i(x):
    return np.asarray(x, dtype=np.int64)


def _cdiv(a, b):
    return (a + b - 1) // b


def group_count(B, L, explicit, gc_probe):
    """wm_group_count"""
    B, L, explicit, gc_probe = np.broadcast_arrays(_i(B), np.maximum(_i(L), 1), _i(explicit) != 0, _i(gc_probe))
    gc = np.where(gc_probe > 0, gc_probe, GROUP_CHUNKS)
    measured = np.minimum(np.where(B < 32, 1, 2), L)
    by_chunks = _cdiv(B, gc)
    rounds = np.maximum(_cdiv(B, DEC_MAXB), L)
    rounds = _cdiv(rounds, L) * L
    G = np.where(~explicit & (gc_probe == 0) & (B < 144), measured, np.where(B <= gc * L, by_chunks, rounds))
    g_min = _cdiv(B, DEC_MAXB)
    return np.where(G < g_min, g_min, np.maximum(G, 1))


def lane_parts(B, L, explicit, d, knob):
    """wm_lane_parts (the knob: WmTuning::lane_parts)"""
    B, L, explicit, d, knob = np.broadcast_arrays(_i(B), _i(L), _i(explicit) != 0, _i(d), _i(knob))
    forced = np.where((B >= 2 * knob) & (B <= knob * DEC_MAXB), knob, 0)
    rule = np.where(d <= 384, np.where((B >= 32) & (B < 48), 2, 0), np.where(d <= 512, np.where((B >= 24) & (B <= 128), 2, 0), 0))
    rule = np.where(explicit | (L < 2), 0, rule)
    return np.where(knob == 1, 0, np.where((knob == 2) | (knob == 3), forced, rule))


def plan(B, N, lanes, explicit, prof_on, no_cu_masks, d, knob_parts, knob_solo, knob_chunks):
    """The composite decision of transcribe_impl: (L, parts, G, n_lanes, kind), each an int64 array over the cases.  The cut
    of case i is balanced_cut(B[i], G[i])."""
    B, N, lanes, explicit, prof_on, no_cu_masks, d, knob_parts, knob_solo, knob_chunks = np.broadcast_arrays(
        _i(B), _i(N), _i(lanes), _i(explicit), _i(prof_on), _i(no_cu_masks), _i(d), _i(knob_parts), _i(knob_solo), _i(knob_chunks))
    L = np.where(prof_on != 0, 1, lanes)
    solo = knob_solo != 0
    parts = np.where((prof_on != 0) | solo | (no_cu_masks != 0) | (N > 1), 0, lane_parts(B, L, explicit, d, knob_parts))
    # candidates: wm_group_count's number for the B * N decoder rows, at least what the row cap asks for, at most one per window
    c_max = DEC_MAXB // N
    G_cand = np.minimum(np.maximum(group_count(B * N, L, explicit, 0), _cdiv(B, c_max)), B)
    G_rows = np.where(parts > 0, parts, group_count(B, L, explicit, knob_chunks))
    G = np.where(N > 1, G_cand, G_rows)
    n_lanes = np.where(solo, 1, np.where(parts > 0, parts, np.minimum(G, L)))
    kind = np.where(solo, SOLO, np.where(parts > 0, PARTS, CLONES))
    return L, parts, G, n_lanes, kind


def balanced_cuts(B, G):
    """wm_balanced_cut of every case, back to back: per case b0[0 .. G) then cg[0 .. G).  Returns (flat, first entry of
    each case)."""
    B, G = _i(B), _i(G)
    start = np.concatenate([[0], np.cumsum(2 * G)[:-1]])
    case = np.repeat(np.arange(len(G)), G)
    g = np.arange(int(G.sum())) - np.repeat(np.cumsum(G) - G, G)
    base, rem = (B // G)[case], (B % G)[case]
    cg = base + (g < rem)
    b0 = g * base + np.minimum(g, rem)
    flat = np.empty(int(2 * G.sum()), dtype=np.int64)
    at = np.repeat(start, G) + g
    flat[at] = b0
    flat[at + np.repeat(G, G)] = cg
    return flat, start


def right_align(prompts, stride, prompt_len, b0, Bg):
    """wm_right_align: (P, table [P][Bg], off [Bg])"""
    P = max(int(prompt_len[b0 + b]) for b in range(Bg))
    table = np.zeros((P, Bg), dtype=np.int64)
    off = np.zeros(Bg, dtype=np.int64)
    for b in range(Bg):
        row = prompts[(b0 + b) * stride:]
        o = P - int(prompt_len[b0 + b])
        off[b] = o
        for t in range(P):
            table[t, b] = row[0 if t < o else t - o]
    return P, table, off


def group_tables(prompts, stride, prompt_len, n_prompt, budgets, sample_ids, b0, Cg, N, want_ids):
    """The pure half of lane_prefill for the group of rows (windows) [b0, b0 + Cg) x N candidates: (P, prompt table [P][Bg],
    offsets [Bg] or None, budgets [Bg] or None, id words or None).  prompt_len None: a uniform call of n_prompt tokens per
    row (stride 0: one prompt for all); budgets / sample_ids None: none."""
    Bg = Cg * N
    off = None
    if prompt_len is not None:
        P, t1, o1 = right_align(prompts, stride, prompt_len, b0, Cg)
        table = np.zeros((P, Bg), dtype=np.int64)
        off = np.zeros(Bg, dtype=np.int64)
        for b in range(Bg):   # every candidate of a window steps through the window's prompt
            off[b] = o1[b // N]
            table[:, b] = t1[:, b // N]
    else:
        P = n_prompt
        table = np.zeros((P, Bg), dtype=np.int64)
        for t in range(P):
            for b in range(Bg):
                table[t, b] = prompts[(b0 + b // N) * stride + t]
    bud = None if budgets is None else np.array([budgets[b0 + b // N] for b in range(Bg)], dtype=np.int64)
    ids = None
    if want_ids and N > 1:   # per row the window's id (given, or its index in the call) and the candidate word
        ids = np.zeros(2 * XIDS_CAND, dtype=np.int64)
        for b in range(Bg):
            ids[b] = sample_ids[b0 + b // N] if sample_ids is not None else b0 + b // N
            ids[XIDS_CAND + b] = b % N
    elif want_ids and sample_ids is not None:
        ids = np.array(sample_ids[b0:b0 + Bg], dtype=np.int64)
    return P, table, off, bud, ids


def group_rows_out(gen, lp, ns, budgets, eot, N, b0, Bg, max_new, tokens, lens, logprobs, no_speech):
    """The plain rows' output loop of the DRAINING branch: gen / lp [max_new][Bg], ns [Bg]; budgets [B] of the call, clamped
    to max_new, or None; writes rows b0 * N .. b0 * N + Bg - 1 of tokens [.][max_new], lens, logprobs (None: not wanted) and
    no_speech [B] (None: not wanted).  The token that stops a row has its log-prob; nothing after it."""
    for b in range(Bg):
        w = b0 + b // N
        o = b0 * N + b
        n = max_new
        if budgets is not None and budgets[w] < n:
            n = int(budgets[w])
        for i in range(n):
            if eot >= 0 and gen[i][b] == eot:
                n = i + 1
                break
        for i in range(max_new):
            tokens[o][i] = gen[i][b] if i < n else eot
        lens[o] = n
        if logprobs is not None:
            for i in range(max_new):
                logprobs[o][i] = lp[i][b] if i < n else 0.0
        if no_speech is not None and b % N == 0:
            no_speech[w] = ns[b]
