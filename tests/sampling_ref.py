"""numpy / f64 restatement of the sampling rules (wm_set_sampling_rules), shared by the sampling-rule
tests, and the seeded generators of the kernel hook's inputs (so that the CPU and the GPU tests look at the same rows).

The rules: A = the admissible ids whose value is above -inf, ordered by descending value, equal values lower id first;
m(n) = exp((v(n) - vmax) * inv_T); the kept set is the shortest prefix of A that satisfies top_k (exactly k), top_p (the shortest
prefix whose mass reaches top_p times the mass of the top_k prefix) and min_p (m(n) >= min_p), never fewer than one id."""
import types

import numpy as np

TOL = 1e-4   # the slack below which a top_p / min_p cut may legitimately fall one way or the other (see kept_detail)


def prepare(v, admissible, inv_T):
    """The order and the masses of a row, which no rule changes: ids of A (ordered), their values, m, the running mass."""
    v = np.asarray(v, dtype=np.float32)
    ok = np.asarray(admissible, dtype=bool) & (v > -np.inf)
    ids = np.nonzero(ok)[0]
    vv = v[ids].astype(np.float64)
    order = np.lexsort((ids, -vv))
    ids, vv = ids[order], vv[order]
    m = np.exp((vv - vv[0]) * float(np.float32(inv_T))) if ids.size else np.zeros(0)
    return types.SimpleNamespace(ids=ids, vv=vv, m=m, cum=np.cumsum(m))


def kept_detail(v, admissible, inv_T, top_k=0, top_p=1.0, min_p=0.0, pre=None):
    """Everything about a row's kept set: ids (all of A, ordered), count, slack, and `accept`: the counts a correct
    implementation in f32 / 2^-40 fixed point may return -- {count} when slack > TOL.

    slack: the smaller relative distance between a threshold and the two values next to its cut -- for top_p the cumulative
    masses just before and just after the cut against top_p * Z_k, over Z (the mass of A); for min_p the masses m of the last
    kept and the first dropped id against min_p, over min_p.  inf when neither rule is active or neither cut has a neighbour."""
    pre = prepare(v, admissible, inv_T) if pre is None else pre
    ids, vv, m, cum = pre.ids, pre.vv, pre.m, pre.cum
    out = types.SimpleNamespace(ids=ids, count=0, slack=np.inf, accept={0}, m=m, tie=False)
    if ids.size == 0:
        return out
    n = ids.size
    Z = cum[-1]
    ck = min(int(top_k), n) if top_k > 0 else n
    slack = np.inf
    p_lo = p_hi = m_lo = m_hi = n
    if top_p < 1.0:
        thr = float(np.float32(top_p)) * cum[ck - 1]
        cp = int(np.searchsorted(cum, thr, side="left")) + 1          # the first prefix whose mass is >= thr
        cp = min(cp, n)
        before = cum[cp - 2] if cp >= 2 else -np.inf
        slack = min(slack, (thr - before) / Z, (cum[cp - 1] - thr) / Z)
        # the prefixes that reach thr -+ TOL Z first
        p_lo = min(int(np.searchsorted(cum, thr - TOL * Z, side="left")) + 1, n)
        p_hi = min(int(np.searchsorted(cum, thr + TOL * Z, side="left")) + 1, n)
    else:
        cp = n
    if min_p > 0.0:
        mp = float(np.float32(min_p))
        cm = int(np.count_nonzero(m >= mp))
        if cm < n:
            slack = min(slack, (mp - m[cm]) / mp)
        slack = min(slack, (m[cm - 1] - mp) / mp) if cm >= 1 else slack
        m_lo = int(np.count_nonzero(m >= mp * (1 + TOL)))
        m_hi = int(np.count_nonzero(m >= mp * (1 - TOL)))
    else:
        cm = n
    count = max(1, min(ck, cp, cm))
    out.ids, out.count, out.slack, out.m = ids, count, slack, m
    out.accept = {max(1, min(ck, a, b)) for a in range(p_lo, p_hi + 1) for b in range(m_lo, m_hi + 1)}
    out.accept.add(count)
    out.tie = count < n and vv[count - 1] == vv[count]      # the cut falls among equal values
    return out


def kept(v, admissible, inv_T, top_k=0, top_p=1.0, min_p=0.0):
    """(ordered ids of A, count, slack): the kept set is ids[:count]."""
    d = kept_detail(v, admissible, inv_T, top_k, top_p, min_p)
    return d.ids, d.count, d.slack


def admissible_set(v, V, suppress, rng_row):
    """The admissible set of the kernel hook's row: (mask [V], forced, sum-rule gap).  rng_row None: every id that is not
    suppressed.  Else (text_lo, text_hi, ts_lo, ts_hi) and the sum rule on the raw values: the timestamps alone when their
    log-sum-exp exceeds the best text value, or when there is no text."""
    ok = np.ones(V, bool)
    ok[list(suppress)] = False
    idx = np.arange(V)
    if rng_row is None:
        return ok, False, np.inf
    tl, th, sl, sh = (int(x) for x in rng_row)
    text, ts = ok & (idx >= tl) & (idx < th), ok & (idx >= sl) & (idx < sh)
    forced, gap = False, np.inf
    if ts.any():
        forced = True
        if text.any():
            r = np.asarray(v, np.float64)
            mx = r[ts].max()
            gap = (mx + np.log(np.exp(r[ts] - mx).sum())) - r[text].max() if np.isfinite(mx) else -np.inf
            forced = gap > 0
    return (ts if forced else (text | ts)), forced, gap


# ---------------------------------------------------------------------------------------------------------------- inputs
KINDS = ("normal1", "normal8", "equal", "spike", "one", "none", "forced", "cut_inf")
GEOM = {16: 12, 1024: 900, 51865: 50364}      # V -> ts_begin
RULES = ([(k, 1.0, 0.0) for k in (1, 2, 50, 1000, "V", "V+7")] + [(0, p, 0.0) for p in (1e-6, 0.5, 0.9, 0.999)] +
         [(0, 1.0, mp) for mp in (0.05, 0.5)] + [(50, 0.9, 0.05)])
POOL_ROWS = 128


def rules_for(V):
    return [(V if k == "V" else V + 7 if k == "V+7" else k, p, mp) for k, p, mp in RULES]


def hook_inputs(V, seed=0):
    """The pool of 128 rows of one vocabulary, 16 per kind (row r is of kind KINDS[r % 8]): logits f32 [128][V], the call's
    suppress list, rng i32 [128][4], ts_begin, kinds, sample ids.  Text ranges lie below ts_begin, timestamp ranges at or above.
    The first 4 rows of the normal, spike and forced kinds range over the whole vocabulary; the other 12 have NARROW ranges (7 ..
    40 text ids, up to 8 timestamps): in a wide row every id near the end of a nucleus holds less than TOL of the mass, so its
    top_p cut is inside the slack by construction, and the exact checks need rows where it is not."""
    g = np.random.default_rng(1000 * V + seed)
    tsb = GEOM[V]
    lg = np.zeros((POOL_ROWS, V), np.float32)
    rng = np.zeros((POOL_ROWS, 4), np.int32)
    # suppressed everywhere: ids that the cut_inf rows place at the top
    sup = sorted({1, 5, tsb - 1, min(tsb + 1, V - 1)})
    kinds = []
    for r in range(POOL_ROWS):
        kind = KINDS[r % len(KINDS)]
        kinds.append(kind)
        row = g.standard_normal(V)
        rg = (0, tsb, tsb, V)
        if r // len(KINDS) >= 4:
            w, a, c = int(g.integers(7, 41)), int(g.integers(0, max(1, tsb - 40))), int(g.integers(0, max(1, V - tsb - 8)))
            rg = (a, min(a + w, tsb), tsb + c, min(tsb + c + 8, V))
        if kind == "normal8":
            row *= 8
        elif kind == "equal":
            row[:] = g.standard_normal()
            rg = (0, tsb, tsb, tsb)            # text only: every value equal, the cut falls among ties
        elif kind == "spike":
            row[int(g.integers(rg[0], rg[1]))] += 30
        elif kind == "one":
            a = int(g.choice([i for i in range(tsb) if i not in sup]))
            rg = (a, a + 1, tsb, tsb)
        elif kind == "none":
            rg = (0, 0, tsb, tsb)
        elif kind == "forced":
            rg = (3, 3, rg[2], rg[3])
        elif kind == "cut_inf":
            fin = g.choice(tsb, size=max(5, min(40, tsb // 2)), replace=False)
            keep = row[fin].copy()
            row[:tsb] = -np.inf
            row[fin] = keep
            row[sup] = 50.0                   # suppressed ids above everything
            rg = (0, tsb, tsb, tsb)
        lg[r] = row.astype(np.float32)
        rng[r] = rg
    ids = (g.integers(0, 2 ** 32, size=POOL_ROWS, dtype=np.uint64)).astype(np.uint32)
    return types.SimpleNamespace(V=V, ts_begin=tsb, logits=lg, suppress=sup, rng=rng, kinds=kinds, sample_ids=ids)


def pool_reference(inp, inv_T, rules):
    """kept_detail of every row of the pool under every rule set: {rule: [detail per row]}, plus the rows' admissible sets."""
    R = inp.logits.shape[0]
    sets = [admissible_set(inp.logits[r], inp.V, inp.suppress, inp.rng[r]) for r in range(R)]
    pre = [prepare(inp.logits[r], sets[r][0], inv_T) for r in range(R)]
    return sets, {rule: [kept_detail(None, None, inv_T, *rule, pre=pre[r]) for r in range(R)] for rule in rules}


# ------------------------------------------------------------------------------------------------ what the GPU test checks
SUB17 = list(range(8)) + list(range(32, 40)) + [64]      # every kind, with wide and with narrow ranges


def checked_cases(V):
    """Every launch tests/test_sampling_rules_kernel_gpu.py checks against the restatement, as (T, timestamp rules on, rule, rows):
    the whole pool under each of the thirteen rule sets at T = 1, and 17 rows at T = 2 and without timestamp rules.  (Its subsets
    and permutations repeat rows of the first kind.)  The CPU test holds the 5 % cap over exactly these (row, rule) cases."""
    out = [(1.0, True, rule, list(range(POOL_ROWS))) for rule in rules_for(V)]
    out += [(2.0, True, rule, SUB17) for rule in ((1000, 1.0, 0.0), (V + 7, 1.0, 0.0), (0, 0.9, 0.0))]
    # (without timestamp rules every id is admissible: at 51 865 ids each holds far less than TOL of Z, so a nucleus and a
    # low min_p cut inside the slack by construction there -- those rules are the pool's, on its narrow rows)
    out += [(1.0, False, rule, SUB17) for rule in ((50, 1.0, 0.0), (1000, 1.0, 0.0), (0, 1.0, 0.5))]
    return out


def case_reference(inp, T, with_rng, rule, rows, cache):
    """kept_detail of `rows` for one checked case; `cache` (a dict) keeps each row's order and masses per (T, with_rng)."""
    inv_T = float(np.float32(1.0 / T))
    out = []
    for r in rows:
        key = (T, with_rng, r)
        if key not in cache:
            adm = admissible_set(inp.logits[r], inp.V, inp.suppress, inp.rng[r] if with_rng else None)
            cache[key] = (adm, prepare(inp.logits[r], adm[0], inv_T))
        out.append(kept_detail(None, None, inv_T, *rule, pre=cache[key][1]))
    return out
