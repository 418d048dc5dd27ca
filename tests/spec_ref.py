"""Speculative decoding (wm_transcribe_mel_speculative) restated in plain Python: the group cut, the
width of a verify step, the arithmetic of one round (csrc/spec_round.h, tx_plan.cpp wm_spec_round) and -- from them -- the walk
of a whole call over a script of proposals, which gives the statistics the library must report; the timestamp rules' state
(dec_close.h ts_advance) and, over plain lists, the adopt, stage and commit kernels of spec.hip.  No numpy in the rules: the
tests compare these against the library's pure functions (wmdbg_spec_*) and its kernels."""

DEC_MAXB = 128          # WM_DEC_MAXB
MAX_DRAFT_LEN = 7       # WM_MAX_DRAFT_LEN
DEFAULT_GROUP = 128     # tx_plan.cpp kSpecGroup: the whole call, up to the row bound
NO_CUT = 1 << 30


def balanced_cut(B, G):
    base, rem = divmod(B, G)
    cg = [base + (1 if g < rem else 0) for g in range(G)]
    b0 = [g * base + min(g, rem) for g in range(G)]
    return b0, cg


def spec_groups(B, k, spec_group=0):
    """(b0, cg) of the decode groups of B windows at draft length k"""
    cap = max(1, DEC_MAXB // (k + 1))
    size = min(cap, spec_group if spec_group > 0 else DEFAULT_GROUP)
    return balanced_cut(B, -(-B // size))


def spec_width(k, bound, last):
    room = last - bound + 1
    return 0 if room < 1 else min(k + 1, room)


def window_own(accepted, eot_at, left):
    m = accepted + 1
    if eot_at >= 0:
        m = min(m, eot_at + 1)
    return max(0, min(m, left))


def window_stops(m, eot_at, left):
    return (0 <= eot_at < m) or left <= m


def window_ask(accepted, eot_at, left):
    return NO_CUT if window_stops(window_own(accepted, eot_at, left), eot_at, left) else accepted + 1


def spec_round(w, accepted, live, eot_at, left):
    """One round of a group whose verify step had w rows per window.  Per window: accepted = leading rows whose winner
    equals the proposal, live, eot_at = index of the first end-of-text among its own accepted + 1 tokens (-1: none), left =
    tokens its budget still allows.  Returns (n, live_out, inc) with inc[c] = (rounds, proposed, accepted, kept) increments."""
    G = len(accepted)
    asks = [window_ask(accepted[c], eot_at[c], left[c]) for c in range(G) if live[c]]
    n = min(min(asks), w) if asks else 0
    live_out, inc = [0] * G, [(0, 0, 0, 0)] * G
    for c in range(G):
        if not live[c]:
            continue
        own = window_own(accepted[c], eot_at[c], left[c])
        m = min(n, own)
        live_out[c] = 0 if window_stops(m, eot_at[c], left[c]) else 1
        inc[c] = (1, w - 1, min(accepted[c], own), min(accepted[c], m))
    return n, live_out, inc


# ---------------------------------------------------------------- the timestamp rules' state (model.h WmTsDev, dec_close.h)
def ts_start(ts_begin, n_vocab, max_initial):
    """(hist, rng) before the first sampled token, as ts_init_kernel leaves them: no text token may open the transcript and
    the first timestamp is at most max_initial (< 0: unlimited).  hist = (n_sampled, last_is_ts, prev_is_ts, last_ts)."""
    hi = ts_begin + max_initial + 1 if 0 <= max_initial and ts_begin + max_initial + 1 < n_vocab else n_vocab
    return (0, 0, 1, -1), (0, 0, ts_begin, hi)


def ts_advance(hist, tok, ts_begin, eot, n_vocab):
    """dec_close.h ts_advance: `tok` was sampled behind the history `hist`.  Returns (hist', (text_lo, text_hi, ts_lo, ts_hi)),
    the ranges of allowed text and timestamp ids at the next position (ApplyTimestampRules without the sum rule).  An empty
    timestamp range behind a closed pair is stated the way the device states it: ts_hi = ts_begin, ts_lo still the floor."""
    n, last_is_ts, _, last_ts = hist
    is_ts = tok >= ts_begin
    penultimate_ts = n < 1 or last_is_ts != 0        # of the history WITH tok: len(seq) < 2 or seq[-2] >= ts_begin
    newest = tok if is_ts else last_ts
    text_lo, text_hi, ts_lo, ts_hi = 0, ts_begin, ts_begin, n_vocab
    if is_ts and penultimate_ts:
        ts_hi = ts_begin                             # a pair was closed: no timestamp next
    elif is_ts:
        text_lo = eot                                # an opening timestamp: its partner, or end-of-text
    if newest >= 0:                                  # timestamps do not decrease, and advance unless they close a pair
        ts_lo = max(ts_lo, newest if (is_ts and not penultimate_ts) else newest + 1)
    return (n + 1, 1 if is_ts else 0, last_is_ts, newest), (text_lo, text_hi, ts_lo, ts_hi)


def ts_replay(hist, rng, toks, ts):
    """(hist, rng) advanced along toks with the rule parameters ts = (ts_begin, eot, n_vocab, max_initial)"""
    for t in toks:
        hist, rng = ts_advance(hist, t, ts[0], ts[1], ts[2])
    return tuple(hist), tuple(rng)


def rule_histories(alphabet, ts, max_len=5):
    """Every token history of length 0 .. max_len over `alphabet` that the rules allow -- each token inside the ranges behind
    the tokens in front of it --, shortest first, in the alphabet's order: a list of (tokens, hist, rng), and the number of
    histories of those lengths that were left out."""
    out, level = [], [((),) + ts_start(ts[0], ts[2], ts[3])]
    for _ in range(max_len + 1):
        out += level
        level = [(toks + (t,),) + ts_advance(h, t, ts[0], ts[1], ts[2]) for toks, h, r in level for t in alphabet
                 if r[0] <= t < r[1] or r[2] <= t < r[3]]
    return out, sum(len(alphabet) ** n for n in range(max_len + 1)) - len(out)


# ---------------------------------------------------------------- the bookkeeping kernels of a round (spec.hip), on plain lists
# A state `st` is a dict of nested lists in the device's shapes: tseq / dseq [n_ctx][G], the [.][4] state arrays (tts_hist,
# tts_rng, dts_hist, dts_rng, chist, crng, dchist, dcrng, stats), wtok / wlp [G * w], acc / done / budget [G], logprob
# [max_new][G], script [G][max_new] or None, pos.  tts / dts: a model's rule parameters (ts_begin, eot, n_vocab, max_initial),
# None = its rules are off.  Each function returns a dict of the arrays the kernel writes, whole and new; st is not modified.
def _copy(a):
    return [list(r) if isinstance(r, (list, tuple)) else r for r in a]


def adopt_ref(st, G, n_prompt, tts, dts):
    """The draft adopts the target's first generated token (position n_prompt): its token buffer takes it, the statistics
    start at zero, the target's state after its first close becomes the committed one, and the draft's state -- running and
    committed -- is the initial history advanced by that token with the draft's own parameters."""
    out = {k: _copy(st[k]) for k in ("dseq", "stats")}
    for c in range(G):
        out["dseq"][n_prompt][c] = st["tseq"][n_prompt][c]
        out["stats"][c] = [0, 0, 0, 0]
    if tts is not None:
        out["chist"], out["crng"] = _copy(st["chist"]), _copy(st["crng"])
        for c in range(G):
            out["chist"][c], out["crng"][c] = list(st["tts_hist"][c]), list(st["tts_rng"][c])
    if dts is not None:
        for k in ("dts_hist", "dts_rng", "dchist", "dcrng"):
            out[k] = _copy(st[k])
        for c in range(G):
            h, r = ts_advance(ts_start(dts[0], dts[2], dts[3])[0], st["tseq"][n_prompt][c], dts[0], dts[1], dts[2])
            out["dts_hist"][c], out["dchist"][c] = list(h), list(h)
            out["dts_rng"][c], out["dcrng"][c] = list(r), list(r)
    return out


def stage_ref(st, G, w, n_prompt, n_ctx, max_new, n_vocab, tts):
    """The proposals d[0 .. w - 1) of window c go to positions pos + 1 .. pos + w - 1 of the target's token buffer, as far as
    the context reaches: the script's entry for that generated index where there is one, else the draft's token at that
    position, clamped into the vocabulary.  Row (c, s) of the verify step gets the ranges behind d[0 .. s), replayed from the
    window's committed state; row (c, 0) the committed ranges themselves."""
    pos = st["pos"]
    out = {"tseq": _copy(st["tseq"])}
    if tts is not None:
        out["tts_rng"] = _copy(st["tts_rng"])
    for c in range(G):
        d = []
        for p in range(pos + 1, min(pos + w, n_ctx)):
            gi = p - n_prompt
            t = st["script"][c][gi] if st["script"] is not None and 0 <= gi < max_new else st["dseq"][p][c]
            d.append(min(max(t, 0), n_vocab - 1))
            out["tseq"][p][c] = d[-1]
        if tts is not None:
            out["tts_rng"][c * w] = list(st["crng"][c])
            for s in range(1, len(d) + 1):
                out["tts_rng"][c * w + s] = list(ts_replay(st["chist"][c], st["crng"][c], d[:s], tts)[1])
    return out


def commit_ref(st, G, w, n_prompt, n_ctx, max_new, eot, pad_tok, tts, dts):
    """The lockstep cut (spec_round) and what follows from it.  A live window keeps m = min(n, its own tokens) winners and their
    log-probs and pads up to n (token pad_tok, log-prob 0; log-probs only inside max_new); a frozen window pads all n.  The
    target's committed state advances along the m kept tokens.  Both positions become pos + n, the draft's token buffer takes
    the target's token there, and the draft's state, running and committed, is its committed one advanced along the n tokens
    the group moved by, with the draft's parameters.  wlp values are copied as given (the tests pass bit patterns)."""
    pos = st["pos"]
    g0 = pos + 1 - n_prompt
    acc = [st["acc"][c] for c in range(G)]
    live = [1 if st["done"][c] == 0 else 0 for c in range(G)]
    eot_at, left = [-1] * G, [0] * G
    for c in range(G):
        if not live[c]:
            continue
        own = st["wtok"][c * w:c * w + acc[c] + 1]
        if eot >= 0 and eot in own:
            eot_at[c] = own.index(eot)
        left[c] = min(max_new, st["budget"][c] if st["budget"] is not None else max_new) - g0
    n, live_out, inc = spec_round(w, acc, live, eot_at, left)
    out = {k: _copy(st[k]) for k in ("tseq", "dseq", "logprob", "done", "stats")}
    for k in ("chist", "crng") if tts is not None else ():
        out[k] = _copy(st[k])
    for k in ("dts_hist", "dts_rng", "dchist", "dcrng") if dts is not None else ():
        out[k] = _copy(st[k])
    for c in range(G):
        m = min(n, window_own(acc[c], eot_at[c], left[c])) if live[c] else 0
        toks = st["wtok"][c * w:c * w + m] + [pad_tok] * (n - m)
        lps = st["wlp"][c * w:c * w + m] + [0] * (n - m)
        for i in range(n):
            out["tseq"][pos + 1 + i][c] = toks[i]
            if 0 <= g0 + i < max_new:
                out["logprob"][g0 + i][c] = lps[i]
        if live[c]:
            out["done"][c] = 0 if live_out[c] else 1
            out["stats"][c] = [a + b for a, b in zip(st["stats"][c], inc[c])]
        if tts is not None and m > 0:
            h, r = ts_replay(st["chist"][c], st["crng"][c], toks[:m], tts)
            out["chist"][c], out["crng"][c] = list(h), list(r)
        if n > 0:
            out["dseq"][pos + n][c] = toks[n - 1]
        if dts is not None:
            h, r = ts_replay(st["dchist"][c], st["dcrng"][c], toks, dts)
            out["dts_hist"][c], out["dchist"][c] = list(h), list(h)
            out["dts_rng"][c], out["dcrng"][c] = list(r), list(r)
    n_live = sum(live_out)
    out.update(n_live=n_live, round=[n_live, pos + n], tpos=pos + n, dpos=pos + n)
    return out


def walk_group(plain, lens, script, n_prompt, max_new, k, eot, budgets=None, trace=None):
    """The rounds of ONE decode group.  plain [G][max_new] / lens [G]: the plain call's tokens (the target's own choices up to
    a window's end), script [G][max_new]: the proposals by generated index, budgets [G] or None.  Returns per window
    (rounds, proposed, accepted, kept), following the host loop of spec_group (transcribe.cpp): at most two rounds ahead of
    the device, the width from an upper bound on the position.  trace (a list): per round (w, live before, accepted, n)."""
    G = len(plain)
    stats = [[0, 0, 0, 0] for _ in range(G)]
    if max_new < 2:
        return [tuple(s) for s in stats]
    bud = [min(max_new, budgets[c]) if budgets is not None else max_new for c in range(G)]
    # after the first token (a plain step): a window is done if that token stopped it
    live = [0 if ((eot >= 0 and plain[c][0] == eot) or bud[c] <= 1) else 1 for c in range(G)]
    last = n_prompt + max_new - 2
    pos, results, widths = n_prompt, [], []
    rounds = seen = 0
    bound, stopped = n_prompt, False
    while True:
        w = spec_width(k, bound, last)
        while seen < rounds and (rounds - seen >= 2 or w == 0):
            n_live, p = results[seen]
            stopped = stopped or n_live == 0
            seen += 1
            bound = p + sum(widths[seen:rounds])
            w = spec_width(k, bound, last)
        if stopped or w == 0:
            break
        g0 = pos + 1 - n_prompt
        acc, eot_at, left = [0] * G, [-1] * G, [0] * G
        for c in range(G):
            if not live[c]:
                continue
            assert g0 < lens[c], "a live window has tokens left"
            # leading proposals equal to the target's own tokens; what lies behind a window's stopping token is not the target's
            # and is never counted (window_own caps the device's count in the same way)
            a = 0
            while a < min(w - 1, lens[c] - g0) and script[c][g0 + a] == plain[c][g0 + a]:
                a += 1
            acc[c] = a
            left[c] = bud[c] - g0
            if eot >= 0:
                for i in range(min(a + 1, lens[c] - g0)):
                    if plain[c][g0 + i] == eot:
                        eot_at[c] = i
                        break
        was_live = list(live)
        n, live, inc = spec_round(w, acc, live, eot_at, left)
        if trace is not None:
            trace.append((w, was_live, acc, n))
        for c in range(G):
            for j in range(4):
                stats[c][j] += inc[c][j]
        pos += n
        results.append((sum(live), pos))
        widths.append(w)
        bound += w
        rounds += 1
    return [tuple(s) for s in stats]


def walk(plain, lens, script, n_prompt, max_new, k, eot, budgets=None, spec_group=0, trace=None):
    """walk_group over the groups of a call of B windows"""
    B = len(plain)
    b0, cg = spec_groups(B, k, spec_group)
    out = []
    for g in range(len(b0)):
        r = slice(b0[g], b0[g] + cg[g])
        out += walk_group(plain[r], lens[r], script[r], n_prompt, max_new, k, eot, None if budgets is None else budgets[r], trace)
    return out
