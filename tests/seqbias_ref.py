"""numpy restatement of the sequence bias (wm_set_sequence_bias), shared by the sequence-bias tests.

History g[0 .. k): the tokens a row has GENERATED in the call (the prompt is excluded), as in repeat_ref.py.
  entries : sequences s[0 .. n), 1 <= n <= 32, with a bias (finite or -inf); the last token < eot, the others in [0, V).
  match   : n == 1, or k >= n - 1 and g[k - n + 1 .. k) == s[0 .. n - 1).
  total(t): float32 sum from +0.0 of the biases of the matching entries whose last token is t, in TABLE order -- the given
            sequences in order, each followed by its implicit entries.  The logit becomes v[t] + total(t) (one f32 add, for
            every id: v + 0.0 where nothing matches); total == -inf is a ban.
  boost   : a boosted sequence adds its proper prefixes s[0 .. j), j = 1 .. n - 1, as implicit entries with its bias; implicit
            entries with identical tokens merge into the FIRST of them with the maximum bias; one identical to a given sequence
            is dropped, and so is one that ends in an id >= eot (only text ids are ever biased).
A table here is a list of (tuple of tokens, float bias) in table order."""
import math

import numpy as np

MAX_LEN, MAX_ENTRIES = 32, 4096


class Invalid(ValueError):
    pass


def expand(seqs, biases, boost=None, *, eot, V):
    """The checked, expanded table of wm_set_sequence_bias in table order.  seqs: token sequences; biases: one float each;
    boost: one flag each or None.  Raises Invalid where the library answers WM_ERR_INVALID."""
    if not 0 <= eot <= V:
        raise Invalid("eot")
    seqs = [tuple(int(t) for t in s) for s in seqs]
    boost = [False] * len(seqs) if boost is None else [bool(f) for f in boost]
    given = set()
    for s, b, f in zip(seqs, biases, boost):
        b = float(b)
        if not 1 <= len(s) <= MAX_LEN or any(not 0 <= t < V for t in s) or s[-1] >= eot:
            raise Invalid("sequence %r" % (s,))
        if math.isnan(b) or b == math.inf or (f and not math.isfinite(b)):
            raise Invalid("bias %r" % b)
        if s in given:
            raise Invalid("duplicate %r" % (s,))
        given.add(s)
    table, implicit = [], {}
    for s, b, f in zip(seqs, biases, boost):
        b = float(np.float32(b))
        table.append([s, b])
        if not f:
            continue
        for j in range(1, len(s)):
            pre = s[:j]
            if pre[-1] >= eot or pre in given:
                continue
            if pre in implicit:
                implicit[pre][1] = max(implicit[pre][1], b)
                continue
            implicit[pre] = [pre, b]
            table.append(implicit[pre])
    if len(table) > MAX_ENTRIES:
        raise Invalid("%d entries" % len(table))
    return [(s, b) for s, b in table]


def matches(s, g):
    n, k = len(s), len(g)
    return n == 1 or (k >= n - 1 and tuple(int(t) for t in g[k - n + 1:]) == tuple(s[:n - 1]))


def totals(table, g):
    """{id: float32 total} over the ids with at least one matching entry, summed in table order"""
    out = {}
    for s, b in table:
        if matches(s, g):
            out[s[-1]] = np.float32(out.get(s[-1], np.float32(0.0)) + np.float32(b))
    return out


def apply_bias(v, table, g):
    """(float32 row v + total, bool mask of the banned ids) for history g.  A banned id's value is v + (-inf) = -inf."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    tot = np.zeros(v.shape[0], np.float32)
    for t, x in totals(table, g).items():
        tot[t] = x
    with np.errstate(invalid="ignore"):
        out = (v + tot).astype(np.float32)
    return out, tot == -np.inf


def state(table, g, V):
    """What the state kernel leaves for a row: (hit words, ban words, ids ascending, float32 totals, per word the hit bits in the
    words below it = the list index of the word's first hit id)"""
    from repeat_ref import bitmap
    tot = totals(table, g)
    ids = sorted(tot)
    hit = bitmap(ids, V)
    pop = np.array([bin(int(w)).count("1") for w in hit], np.int64)
    woff = (np.cumsum(pop) - pop).astype(np.int32)
    return (hit, bitmap([t for t in ids if tot[t] == -np.inf], V), np.array(ids, np.int32),
            np.array([tot[t] for t in ids], np.float32), woff)


def pack(seqs, biases, boost=None):
    """The arrays of the C call: tokens i32, seq_offsets i32 [n + 1], bias f32 [n], boost u8 [n] or None"""
    toks = np.array([t for s in seqs for t in s], np.int32)
    offs = np.zeros(len(seqs) + 1, np.int32)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return toks, offs, np.array(biases, np.float32), None if boost is None else np.array([1 if f else 0 for f in boost], np.uint8)


def contains(tokens, seq):
    """does the token list contain seq as a contiguous run"""
    t, s = [int(x) for x in tokens], [int(x) for x in seq]
    return any(t[i:i + len(s)] == s for i in range(len(t) - len(s) + 1))
