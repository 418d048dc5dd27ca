"""numpy restatement of the repetition rules (wm_set_repetition_rules), shared by the repetition tests.

History g[0 .. k): the tokens a row has GENERATED in the call (the prompt is excluded).  Only ids < eot are eligible.
  penalty p            : every eligible id that occurs in g, once: v = v > 0 ? v * inv_p : v * p, in float32, with
                         inv_p = float32(1.0 / float64(float32(p))) -- one f32 multiply either way, so numpy gives the bits.
  no-repeat n-gram n   : eligible t is banned iff some i in [0, k - n] has g[i .. i + n - 1) == g[k - n + 1 .. k) and
                         g[i + n - 1] == t.  Nothing is banned for k < n - 1 (nor for k == n - 1: no start exists); n = 1 bans
                         every eligible id of g."""
import numpy as np


def seen_set(g, eot):
    return {int(t) for t in g if 0 <= int(t) < eot}


def ban_set(g, n, eot):
    g = [int(t) for t in g]
    k = len(g)
    if n <= 0 or k < n:
        return set()
    suffix = g[k - n + 1:]            # n - 1 tokens (n = 1: none)
    out = set()
    for i in range(k - n + 1):
        t = g[i + n - 1]
        if 0 <= t < eot and g[i:i + n - 1] == suffix:
            out.add(t)
    return out


def words_of(V):
    """32-bit words of a bitmap over V ids as the library lays it out: the vocabulary padded to 16, then to whole words"""
    return (-(-V // 16) * 16 + 31) // 32


def bitmap(ids, V):
    w = np.zeros(words_of(V), np.uint32)
    for t in ids:
        w[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return w


def inv_p(p):
    return np.float32(1.0 / float(np.float32(p)))


def penalise(v, seen, p):
    """float32 logits row -> the penalised row (float32 arithmetic, one multiply per touched id)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = v.copy()
    idx = np.array(sorted(seen), dtype=np.int64)
    if idx.size:
        x = v[idx]
        out[idx] = np.where(x > 0, x * inv_p(p), x * np.float32(p)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def apply_rules(v, g, p, n, eot):
    """(penalised float32 row, bool mask of the banned ids) for history g"""
    v = penalise(v, seen_set(g, eot), p)
    banned = np.zeros(v.shape[0], bool)
    b = sorted(ban_set(g, n, eot))
    if b:
        banned[b] = True
    return v, banned


def repeated_ngrams(g, n, eot):
    """How many n-grams of g end in an eligible id and repeat an EARLIER n-gram of g: exactly the tokens no_repeat_ngram_size
    = n forbids (0 under the rule, unless a fallback token was taken)."""
    g = [int(t) for t in g]
    count = 0
    for j in range(n - 1, len(g)):
        if not 0 <= g[j] < eot:
            continue
        gram = g[j - n + 1:j + 1]
        if any(g[i:i + n] == gram for i in range(j - n + 1)):
            count += 1
    return count
