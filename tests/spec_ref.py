"""Speculative decoding (wm_transcribe_mel_speculative) restated in plain Python: the group cut, the
width of a verify step, the arithmetic of one round (csrc/spec_round.h, tx_plan.cpp wm_spec_round) and -- from them -- the walk
of a whole call over a script of proposals, which gives the statistics the library must report.  No numpy in the rules: the
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
