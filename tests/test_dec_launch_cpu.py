"""CPU test of the decode step's launch plans (csrc/dec_launch.cpp): every field of wm_plan_attention* / wm_plan_gemv, through
the host-only hooks wmdbg_dec_attn_plan / wmdbg_dec_gemv_plan, against the restatement of the launchers' arithmetic in
tests/dec_launch_ref.py -- for every decode-group size, every model geometry, the whole chip and the sub-chip lanes, under the
product's tuning and under each probe knob.  A case the launcher refuses is compared as a refusal.  No GPU."""
import ctypes

import numpy as np
import pytest

import dec_launch_ref as ref

MODELS = ((6, 384), (8, 512), (12, 768), (16, 1024), (20, 1280))   # (H, d) of tiny / base / small / medium / large
CUS = (256, 128, 88, 80, 8)            # whole chip, the two- and three-part lanes, a one-CU-per-XCD solo lane
ALL_B = tuple(range(1, 129))
FEW_B = (1, 8, 16, 17, 32, 56, 96, 128)
S, T = 1500, 448                       # cross-attention keys, self-attention cache rows
# every (epilogue, LayerNorm) pair the decode step launches (wm_dec_gemv's table)
PAIRS = ((ref.DE_QKV, 1), (ref.DE_QKV_P, 1), (ref.DE_Q, 1), (ref.DE_GELU, 1), (ref.DE_LOGITS, 1), (ref.DE_LOGITS_X, 1),
         (ref.DE_LOGITS_XR, 1), (ref.DE_RESID, 0), (ref.DE_Q, 0))
# each WmTuning field the plans read, at each value its comment documents (wm_tuning.h); the last two have no documented
# value but the default: one other value each, so that the knob is seen to act
KNOBS = (("gemv_tn", 1), ("gemv_tn", 2), ("gemv_tn", 4), ("gemv_nblk", 1), ("gemv_ppw2_nblk", 1), ("gemv_ppw2_nblk", 2),
         ("gemv_no_ppw2", 1), ("prefetch_max_b", 0), ("xattn_no_flat", 1), ("xattn_lds_pad", 0), ("logits_tn", 1), ("logits_tn", 2),
         ("xattn_no_deep", 1), ("xattn_fuse_q", 0), ("xattn_split_below", 192), ("xattn_wgs", 128))
HAS_POS, HAS_PART, HAS_OFF, HAS_PF, SHORT, HAS_LIVE = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    ip = ctypes.POINTER(ctypes.c_int32)
    for f in (lib.wmdbg_dec_attn_plan, lib.wmdbg_dec_gemv_plan):
        f.argtypes = [ip, ctypes.c_int, ip]
        f.restype = ctypes.c_int
    lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.wmdbg_set_tuning(b"reset", 0)
    yield lib
    lib.wmdbg_set_tuning(b"reset", 0)


def table(*axes):
    """the cross product of the axes as int64 columns (first axis slowest)"""
    g = np.meshgrid(*[np.asarray(a, dtype=np.int64) for a in axes], indexing="ij")
    return [c.reshape(-1) for c in g]


def run_hook(fn, width_in, width_out, cols):
    n = len(cols[0])
    a = np.zeros((n, width_in), dtype=np.int32)
    for i, c in cols.items() if isinstance(cols, dict) else enumerate(cols):
        a[:, i] = c
    out = np.full((n, width_out), -1, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    assert fn(a.ctypes.data_as(ip), n, out.ctypes.data_as(ip)) == n
    return out


def compare(out, want, names, what):
    """every column of the hook's output against the restatement; returns the number of cases"""
    n = out.shape[0]
    for i, c in enumerate(names):
        got = out[:, i].astype(np.int64) & 0xffffffff
        exp = np.broadcast_to(want[c], (n,)).astype(np.int64) & 0xffffffff
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, "%s: %s differs in %d of %d cases, first at case %d: plan %d, restatement %d" % (
            what, c, bad.size, n, bad[0], got[bad[0]], exp[bad[0]])
    assert not out[:, len(names):].any()
    return n


def attn_in(form, n, **kw):
    """the hook's input columns (include/whisper_mi355x_debug.h)"""
    idx = dict(B=1, C=2, N=3, H=4, T_stride=5, n_keys=6, nsplit=7, K=8, flags=9, pf_rows=10, pf_k=11, n_cus=12)
    cols = {0: np.full(n, form)}
    for k, v in kw.items():
        cols[idx[k]] = v
    return cols


def cand_shapes(rows):
    """(C, N): N in 1 .. 8, every C with C * N in rows"""
    return [(c, n) for n in range(1, 9) for c in range(1, 129) if c * n <= 128 and c * n in rows]


def attention_cases(dbg, t, Bs):
    """every attention form over the domain; returns (cases compared, cases expected)"""
    fn, done, expect = dbg.wmdbg_dec_attn_plan, 0, 0
    rows = set(Bs)
    shapes = cand_shapes(rows)
    for H, d in MODELS:
        # the cross-attention: nsplit from wm_dec_attn_splits (0 below) and forced
        B, cus, ns, short, warm, live = table(Bs, CUS, (0, 1, 2, 4, 8), (0, 1), (0, 1), (0, 1))
        rule = ref.attn_splits(B, H, t)
        ns = np.where(ns == 0, rule, ns)
        flags = HAS_PART | short * SHORT | warm * HAS_PF | live * HAS_LIVE
        out = run_hook(fn, 16, 16, attn_in(0, len(B), B=B, H=H, T_stride=S, n_keys=S, nsplit=ns, flags=flags, pf_rows=d, pf_k=d, n_cus=cus))
        assert (out[:, 14] == rule).all(), "wm_dec_attn_splits"
        out[:, 14] = 0
        done += compare(out, ref.attention(B, H, S, S, ns, True, warm == 1, d, d, short == 1, cus, t), ref.ATTN_COLS, "cross H=%d" % H)
        expect += len(Bs) * len(CUS) * 5 * 2 * 2 * 2
        # a candidate group
        sh, cus, short, warm, live = table(range(len(shapes)), CUS, (0, 1), (0, 1), (0, 1))
        C, N = np.array([s[0] for s in shapes])[sh], np.array([s[1] for s in shapes])[sh]
        flags = HAS_PART | short * SHORT | warm * HAS_PF | live * HAS_LIVE
        out = run_hook(fn, 16, 16, attn_in(1, len(C), C=C, N=N, H=H, T_stride=S, n_keys=S, flags=flags, pf_rows=d, pf_k=d, n_cus=cus))
        done += compare(out, ref.attention_cand(C, N, H, S, S, True, warm == 1, d, d, short == 1, cus, t), ref.ATTN_COLS, "cand H=%d" % H)
        expect += len(shapes) * len(CUS) * 2 * 2 * 2
        # a panel of the teacher-forced pass
        sh, cus, warm = table(range(len(shapes)), CUS, (0, 1))
        C, w = np.array([s[0] for s in shapes])[sh], np.array([s[1] for s in shapes])[sh]
        out = run_hook(fn, 16, 16, attn_in(4, len(C), C=C, N=w, H=H, T_stride=T, flags=HAS_POS | warm * HAS_PF, pf_rows=d, pf_k=d, n_cus=cus))
        done += compare(out, ref.self_attention_panel(C, w, H, T, True, warm == 1, d, d, t), ref.ATTN_COLS, "panel H=%d" % H)
        expect += len(shapes) * len(CUS) * 2
        # the self-attention, plain and ragged
        B, cus, off, warm, live = table(Bs, CUS, (0, 1), (0, 1), (0, 1))
        flags = HAS_POS | off * HAS_OFF | warm * HAS_PF | live * HAS_LIVE
        out = run_hook(fn, 16, 16, attn_in(3, len(B), B=B, H=H, T_stride=T, n_keys=0, flags=flags, pf_rows=d, pf_k=d, n_cus=cus))
        done += compare(out, ref.self_attention(B, H, T, 0, True, off == 1, warm == 1, d, d, t), ref.ATTN_COLS, "self H=%d" % H)
        expect += len(Bs) * len(CUS) * 2 * 2 * 2
        # the fused query projection: every B, so every B at which wm_dec_xattn_fq_applies flips
        B, cus, short, warm = table(Bs, CUS, (0, 1), (0, 1))
        flags = short * SHORT | warm * HAS_PF
        out = run_hook(fn, 16, 16, attn_in(2, len(B), B=B, H=H, T_stride=S, n_keys=S, K=d, flags=flags, pf_rows=d, pf_k=d, n_cus=cus))
        assert (out[:, 14] == ref.fq_applies(B, H, d, short == 1, t)).all(), "wm_dec_xattn_fq_applies"
        out[:, 14] = 0
        done += compare(out, ref.xattn_fq(B, H, S, S, d, warm == 1, d, d, t), ref.ATTN_COLS, "fq H=%d" % H)
        expect += len(Bs) * len(CUS) * 2 * 2
    return done, expect


def gemv_cases(dbg, t, Bs):
    fn, done, expect = dbg.wmdbg_dec_gemv_plan, 0, 0
    for H, d in MODELS:
        pair, B, K, N, cus, warm, hm = table(range(len(PAIRS)), Bs, (d, 4 * d), (d, 3 * d, 4 * d, 51864, 51865, 51866), CUS, (0, 1), (0, 1))
        epi, ln = np.array([p[0] for p in PAIRS])[pair], np.array([p[1] for p in PAIRS])[pair]
        hm = hm * ((H * B + 7) // 8)    # pairs per XCD of a fused consumer, as the decode step sets it
        out = run_hook(fn, 12, 20, [epi, ln, B, N, K, warm, np.full(len(B), d), np.full(len(B), d), hm, cus])
        done += compare(out, ref.gemv(epi, ln == 1, B, N, K, warm == 1, d, d, hm, cus, t), ref.GEMV_COLS, "gemv d=%d" % d)
        expect += len(PAIRS) * len(Bs) * 2 * 6 * len(CUS) * 2 * 2
    return done, expect


def test_attention_plans_match_the_restatement(dbg):
    done, expect = attention_cases(dbg, ref.TUNING, ALL_B)
    for key, val in KNOBS:
        dbg.wmdbg_set_tuning(b"reset", 0)
        assert dbg.wmdbg_set_tuning(key.encode(), val) == 0
        a, b = attention_cases(dbg, dict(ref.TUNING, **{key: val}), FEW_B)
        done, expect = done + a, expect + b
    dbg.wmdbg_set_tuning(b"reset", 0)
    assert done == expect and done > 250000, (done, expect)


def test_gemv_plans_match_the_restatement(dbg):
    done, expect = gemv_cases(dbg, ref.TUNING, ALL_B)
    for key, val in KNOBS:
        dbg.wmdbg_set_tuning(b"reset", 0)
        assert dbg.wmdbg_set_tuning(key.encode(), val) == 0
        a, b = gemv_cases(dbg, dict(ref.TUNING, **{key: val}), FEW_B)
        done, expect = done + a, expect + b
    dbg.wmdbg_set_tuning(b"reset", 0)
    assert done == expect and done > 1000000, (done, expect)


def test_the_rules_are_exercised_on_both_sides(dbg):
    """The domain above reaches both sides of the rules it is meant to pin (else a comparison of two constants would pass)."""
    t = ref.TUNING
    fn = dbg.wmdbg_dec_attn_plan
    # cacheable versus non-temporal deep loads: 3200 KB of K/V per layer -- base at B = 1 below, small at B = 1 above
    for (H, d), want in (((8, 512), ref.FLAT_DEEP_C), ((12, 768), ref.FLAT_DEEP_NT)):
        ns = int(ref.attn_splits(np.array([1]), H, t)[0])
        out = run_hook(fn, 16, 16, attn_in(0, 1, B=[1], H=H, T_stride=S, n_keys=S, nsplit=ns, flags=HAS_PART, n_cus=256))
        assert ns == 8 and out[0, 0] == 0 and out[0, 1] == want
    # the fused query launch applies somewhere and not everywhere, for every model it is built for
    B = np.arange(1, 129)
    for H, d in MODELS:
        ap = ref.fq_applies(B, H, d, False, t)
        assert ap.any() and not ap.all() and np.count_nonzero(ap[1:] != ap[:-1]) == 2
    # refusals are compared too: the LayerNorm-folded GEMV has no K = 4d form (K / 16 > 80 partial statistics)
    out = run_hook(dbg.wmdbg_dec_gemv_plan, 12, 20, [[ref.DE_GELU], [1], [8], [384], [4 * 384], [0], [0], [0], [0], [256]])
    assert out[0, 0] == ref.WM_ERR_INVALID and not out[0, 1:].any()
    r = ref.gemv(ref.DE_GELU, True, 8, 384, 4 * 384, False, 0, 0, 0, 256, t)
    assert r["rc"] == ref.WM_ERR_INVALID
    # every variant, both GEMV part counts, the row split and all tile-group widths occur under the product's tuning
    seen = set()
    for H, d in MODELS:
        B, ns = table(ALL_B, (1, 8))
        seen |= set(ref.attention(B, H, S, S, ns, True, False, d, d, False, 256, t)["variant"])
        g = ref.gemv(*table((ref.DE_RESID,), (0,), ALL_B, (d,), (d, 4 * d)), False, 0, 0, 0, 256, t)
        seen |= {("ppw", int(v)) for v in g["ppw"]} | {("rs", int(v)) for v in g["row_split"]}
        g = ref.gemv(ref.DE_GELU, True, np.array(ALL_B), 4 * d, d, False, 0, 0, 0, 256, t)
        seen |= {("tn", int(v)) for v in g["tn"]}
    assert {ref.STREAM, ref.FLAT_DEEP_C, ref.FLAT_DEEP_NT, ("ppw", 1), ("ppw", 2), ("rs", 0), ("rs", 1), ("tn", 1), ("tn", 2), ("tn", 4)} <= seen
