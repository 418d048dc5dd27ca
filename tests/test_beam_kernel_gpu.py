"""Kernel-level GPU tests of beam search (csrc/beam.hip) through the debug library's hooks: the per-row list kernel against a
numpy restatement in f64, and the in-place re-parenting of the self-attention K/V cache and the rows' histories against a
numpy gather (bit-level)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIST = 9   # WM_MAX_BEAM + 1
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_beam_topk.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int32, vp, vp, vp]
    c.lib.wmdbg_beam_reorder.argtypes = [vp, vp] + [ctypes.c_int] * 7 + [vp, vp, vp, vp]
    yield c
    c.close()


def _p(a):
    return a.ctypes.data_as(vp)


# ---------------------------------------------------------------- the per-row list
def _lists_np(logits, N, suppress, rng):
    """f64: per row (tokens by descending logit then ascending id, log-probs, sum-rule gap, separation of the listed values)"""
    out = []
    for b in range(logits.shape[0]):
        v = logits[b].astype(np.float64)
        ok = np.ones(v.size, bool)
        ok[suppress] = False
        gap = np.inf
        if rng is not None:
            tl, th, sl, sh = rng[b]
            text = np.zeros(v.size, bool)
            text[tl:th] = True
            ts = np.zeros(v.size, bool)
            ts[sl:sh] = True
            text &= ok
            ts &= ok
            if ts.any():
                m = v[ts].max()
                lse_ts = m + np.log(np.exp(v[ts] - m).sum())
                best_text = v[text].max() if text.any() else -np.inf
                gap = lse_ts - best_text
                if gap > 0:
                    text[:] = False
            ok = text | ts
        ok &= np.isfinite(v)
        ids = np.flatnonzero(ok)
        if ids.size == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0), gap, np.inf))
            continue
        m = v[ids].max()
        lse = m + np.log(np.exp(v[ids] - m).sum())
        order = ids[np.lexsort((ids, -v[ids]))]
        top = order[:N + 1]
        vals = v[order[:N + 2]]
        sep = np.min(-np.diff(vals)) if vals.size > 1 else np.inf
        out.append((top, v[top] - lse, gap, sep))
    return out


def _topk(dbg, logits, N, suppress, rng, ts_begin):
    rows, V = logits.shape
    ln = np.full(rows, -1, np.int32)
    lt = np.full((rows, LIST), -1, np.int32)
    ll = np.full((rows, LIST), np.nan, np.float32)
    sup = np.ascontiguousarray(suppress, np.int32)
    r4 = None if rng is None else np.ascontiguousarray(rng, np.int32)
    st = dbg.lib.wmdbg_beam_topk(dbg.handle, _p(logits), rows, V, N, _p(sup) if sup.size else None, sup.size,
                                 _p(r4) if r4 is not None else None, ts_begin, _p(ln), _p(lt), _p(ll))
    assert st == 0, dbg.lib.wm_last_error()
    return ln, lt, ll


@pytest.mark.parametrize("V,N,rows", [(1024, 5, 10), (51865, 8, 16), (51864, 1, 7), (1030, 3, 6)])
def test_list_kernel_against_numpy(dbg, V, N, rows):
    g = np.random.default_rng(V + N)
    logits = (g.standard_normal((rows, V)) * 3.0).astype(np.float32)
    ts_begin = V - 124
    suppress = np.unique(g.integers(0, V, size=60))
    logits[0, g.integers(0, V, size=20)] = -np.inf          # -inf is never listed
    top3 = np.argsort(-logits[1])[:3]
    logits[1, top3] = logits[1, top3[0]]                    # equal logits at the top: the lower id first
    logits[2, suppress[:5]] = 50.0                          # suppressed ids do not enter, however large
    for rng in (None, "ts"):
        r4 = None
        if rng is not None:
            r4 = np.zeros((rows, 4), np.int32)
            for b in range(rows):
                kind = b % 5
                lo = ts_begin + int(g.integers(0, 60))
                if kind == 0:
                    r4[b] = (0, 0, ts_begin, ts_begin + 21)             # the first token: timestamps only, capped
                elif kind == 1:
                    r4[b] = (0, ts_begin, lo, lo)                       # a closed pair: text only
                elif kind == 2:
                    r4[b] = (ts_begin - 10, ts_begin, lo, V)            # an open timestamp: eot-and-above, or its partner
                else:
                    r4[b] = (0, ts_begin, lo, V)                        # both sides: the sum rule decides
            boost = logits.copy()
            boost[3::5, ts_begin:] += 6.0                                # rows where the timestamps' mass wins
            logits_used = boost
        else:
            logits_used = logits
        ln, lt, ll = _topk(dbg, logits_used, N, suppress, r4, ts_begin)
        want = _lists_np(logits_used, N, suppress, r4)
        exact = forced = near = 0
        for b, (top, lp, gap, sep) in enumerate(want):
            if abs(gap) < 1e-3:       # the sum rule within rounding: either side is right
                near += 1
                continue
            forced += int(gap > 0)
            assert ln[b] == top.size, (b, ln[b], top.size)
            assert np.allclose(ll[b, :ln[b]], lp, rtol=0, atol=2e-4), (b, np.abs(ll[b, :ln[b]] - lp).max())
            assert np.all(np.diff(ll[b, :ln[b]]) <= 0)
            if sep > 1e-5 or b == 1:  # separated values (row 1: exact ties, decided by the id)
                assert list(lt[b, :ln[b]]) == list(top), (b, lt[b], top)
                exact += 1
            else:
                assert set(lt[b, :ln[b] - 1]) <= set(int(t) for t in np.argsort(-logits_used[b])[:N + 8])
        assert exact >= rows - 2 and near <= 1, (exact, near)
        if rng is not None:
            assert forced >= 2
    # short lists: fewer admissible ids than N + 1
    few = np.full((N, V), -np.inf, np.float32)
    few[:, 7] = 1.0
    few[:, 3] = 1.0
    ln, lt, ll = _topk(dbg, few, N, [], None, ts_begin)
    assert np.all(ln == min(2, N + 1)) and np.all(lt[:, 0] == 3)
    few[:] = -np.inf
    ln, lt, ll = _topk(dbg, few, N, [], None, ts_begin)
    assert np.all(ln == 0)


# ---------------------------------------------------------------- the re-parenting
def _maps(g, windows, N):
    src = np.zeros((windows, N), np.int32)
    for w in range(windows):
        kind = w % 4
        if kind == 0:
            src[w] = np.arange(N)                                  # the identity: nothing moves
        elif kind == 1:
            src[w] = np.roll(np.arange(N), 1)                      # a rotation: every row is read and written
        elif kind == 2:
            src[w] = int(g.integers(0, N))                         # all from one beam
        else:
            src[w] = g.integers(0, N, size=N)                      # anything
    return src


@pytest.mark.parametrize("windows,N,H,pos", [(5, 1, 6, 0), (2, 8, 6, 447), (2, 8, 20, 0), (6, 5, 6, 100), (4, 2, 20, 447),
                                             (16, 8, 6, 17)])
def test_reorder_kernel_against_a_numpy_gather(dbg, windows, N, H, pos):
    g = np.random.default_rng(windows * 1000 + N * 100 + H + pos)
    L2, T, rows = 2, 448, windows * N
    n_prompt = 1 if pos < 3 else 3
    cache = g.integers(0, 65536, size=(L2, rows, H, T, 64), dtype=np.uint16)
    seq = g.integers(0, 1000, size=(T, rows)).astype(np.int32)
    lp = g.standard_normal((T, rows)).astype(np.float32)
    src = _maps(g, windows, N)
    wdone = np.zeros(windows, np.int32)
    if windows >= 4:
        wdone[[1, 3]] = 1          # windows that have just left: histories move, caches do not
    want_c, want_s, want_l = cache.copy(), seq.copy(), lp.copy()
    gi = pos + 1 - n_prompt        # the histories below this index follow their beams
    for w in range(windows):
        for k in range(N):
            a, b = w * N + k, w * N + int(src[w, k])
            if not wdone[w]:
                want_c[:, a, :, :pos + 1] = cache[:, b, :, :pos + 1]
            want_s[n_prompt:n_prompt + gi, a] = seq[n_prompt:n_prompt + gi, b]
            want_l[:gi, a] = lp[:gi, b]
    got_c, got_s, got_l = cache.copy(), seq.copy(), lp.copy()
    st = dbg.lib.wmdbg_beam_reorder(dbg.handle, _p(got_c), L2, rows, H, T, N, pos, n_prompt, _p(src), _p(wdone), _p(got_s), _p(got_l))
    assert st == 0, dbg.lib.wm_last_error()
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32))
    if N > 1:
        assert not np.array_equal(want_c, cache) or windows < 2
