"""numpy restatement of the constraint (wm_set_constraint): validation, delta, the fold over a history, the
allowed set of a state, the ban words given incoming ban words, and the two builders.  No GPU, no library: the tests hold the
library and the kernels to this file, and test_constraint_cpu.py holds this file to brute force."""
import numpy as np

MAX_STATES, MAX_EDGES = 4096, 65536
DEAD = -1


class Automaton:
    def __init__(self, edge_beg, edge_tok, edge_next, def_next, accept, eot):
        self.edge_beg = np.asarray(edge_beg, np.int64).reshape(-1)
        self.edge_tok = np.asarray(edge_tok, np.int64).reshape(-1)
        self.edge_next = np.asarray(edge_next, np.int64).reshape(-1)
        self.def_next = np.asarray(def_next, np.int64).reshape(-1)
        self.accept = np.asarray(accept, np.int64).reshape(-1)
        self.eot = int(eot)

    @property
    def S(self):
        return self.def_next.size

    def arrays(self):
        """the arguments of wm_set_constraint / the hooks, as contiguous arrays of the ABI's types"""
        return (np.ascontiguousarray(self.edge_beg, np.int32), np.ascontiguousarray(self.edge_tok if self.edge_tok.size else [0], np.int32),
                np.ascontiguousarray(self.edge_next if self.edge_next.size else [0], np.int32), np.ascontiguousarray(self.def_next, np.int32),
                np.ascontiguousarray(self.accept, np.uint8))

    def edges(self, s):
        a, b = int(self.edge_beg[s]), int(self.edge_beg[s + 1])
        return self.edge_tok[a:b], self.edge_next[a:b]


def invalid(a, n_vocab):
    """None for a valid automaton, else the rule of the header it breaks (a short name)."""
    S = a.S
    if S < 1 or S > MAX_STATES:
        return "states"
    if not (0 <= a.eot < n_vocab):
        return "eot"
    if a.edge_beg.size != S + 1 or a.edge_beg[0] != 0:
        return "offsets"
    if np.any(np.diff(a.edge_beg) < 0):
        return "offsets"
    E = int(a.edge_beg[-1])
    if E > MAX_EDGES:
        return "edges"
    if a.edge_tok.size < E or a.edge_next.size < E:
        return "offsets"
    for s in range(S):
        d = int(a.def_next[s])
        if d < -1 or d >= S:
            return "def_next"
        tok, nxt = a.edges(s)
        if np.any(tok < 0) or np.any(tok >= a.eot):
            return "edge token"
        if np.any(np.diff(tok) <= 0):
            return "ascending"
        if np.any(nxt < -1) or np.any(nxt >= S):
            return "edge_next"
        if d < 0 and np.any(nxt < 0):
            return "explicit -1"
        if d < 0 and not np.any(nxt >= 0) and not a.accept[s]:
            return "stuck"
    return None


def delta(a, s, t):
    """the state after token t in state s"""
    if t < 0 or t >= a.eot or s == DEAD:        # transparent: timestamps, specials, the padding eot; the dead state stays dead
        return s
    tok, nxt = a.edges(s)
    i = np.flatnonzero(tok == t)
    return int(nxt[i[0]]) if i.size else int(a.def_next[s])


def fold(a, start, hist):
    s = int(start)
    for t in hist:
        s = delta(a, s, int(t))
    return s


def allowed(a, s):
    """bool [eot + 1]: the ids of [0, eot] state s allows"""
    ok = np.zeros(a.eot + 1, bool)
    if s == DEAD:
        ok[a.eot] = True
        return ok
    if a.def_next[s] >= 0:
        ok[:a.eot] = True
    tok, nxt = a.edges(s)
    ok[tok] = nxt >= 0
    ok[a.eot] = bool(a.accept[s])
    return ok


def words_of(V):
    return ((V + 15) // 16 * 16 + 31) // 32


def ban_words(a, start, hist, ban_in):
    """the row's ban words u32 [words] after the launch: ban_in | the ids of [0, eot] the reached state does not allow; a row on
    start -1 keeps ban_in.  -> (words, state)"""
    out = np.array(ban_in, np.uint32, copy=True)
    if start < 0:
        return out, None
    s = fold(a, start, hist)
    bad = np.flatnonzero(~allowed(a, s))
    np.bitwise_or.at(out, bad >> 5, (np.uint32(1) << (bad & 31).astype(np.uint32)))
    return out, s


def banned_mask(a, start, hist, V):
    """bool [V]: the ids the constraint bans for a row with this history (none above eot; none for start -1)"""
    m = np.zeros(V, bool)
    if start >= 0:
        m[:a.eot + 1] = ~allowed(a, fold(a, start, hist))
    return m


# ------------------------------------------------------------------ the builders
def from_choices(choices, eot, repeat=False):
    """binding.constraint_from_choices restated over a dict trie"""
    trie = {(): {}}                      # prefix -> {token: prefix of the target}
    acc = {(): bool(repeat)}
    for c in choices:
        c = tuple(int(t) for t in c)
        for i in range(len(c)):
            last = i == len(c) - 1
            tgt = () if (repeat and last) else c[:i + 1]
            trie[c[:i]][c[i]] = tgt
            trie.setdefault(tgt, {})
            acc.setdefault(tgt, False)
            if last and not repeat:
                acc[tgt] = True
    order = [()] + sorted((p for p in trie if p), key=lambda p: (len(p), p))   # any numbering: the language does not depend on it
    num = {p: i for i, p in enumerate(order)}
    beg, tok, nxt = [0], [], []
    for p in order:
        for t in sorted(trie[p]):
            tok.append(t)
            nxt.append(num[trie[p][t]])
        beg.append(len(tok))
    return Automaton(beg, tok, nxt, [-1] * len(order), [acc[p] for p in order], eot)


def join(automata):
    beg, tok, nxt, dn, acc, starts = [0], [], [], [], [], []
    for a in automata:
        s0, e0 = len(dn), len(tok)
        starts.append(s0)
        beg += [int(x) + e0 for x in a.edge_beg[1:]]
        tok += [int(x) for x in a.edge_tok]
        nxt += [int(x) + s0 if x >= 0 else -1 for x in a.edge_next]
        dn += [int(x) + s0 if x >= 0 else -1 for x in a.def_next]
        acc += [int(x) for x in a.accept]
    return Automaton(beg, tok, nxt, dn, acc, automata[0].eot), starts


def of_binding(c, eot):
    """a binding.Constraint as an Automaton"""
    return Automaton(c.edge_beg, c.edge_tok, c.edge_next, c.def_next, c.accept, eot)


def language(a, start, alphabet, max_len):
    """every string over `alphabet` (text ids) up to max_len that the automaton generates: always an allowed id, ending where eot
    is allowed"""
    out, frontier = set(), [((), int(start))]
    for _ in range(max_len + 1):
        nxt = []
        for w, s in frontier:
            ok = allowed(a, s)
            if ok[a.eot]:
                out.add(w)
            for t in alphabet:
                if ok[t]:
                    nxt.append((w + (t,), delta(a, s, t)))
        frontier = nxt
    return {w for w in out if len(w) <= max_len}
