"""Restatement of the decode step's launch arithmetic, as the launchers of csrc/dec_kernels.hip stated it before the rules
moved into csrc/dec_launch.cpp: one function per launcher, in the launcher's own order, so that it reads against the C++ it
restates.  tests/test_dec_launch_cpu.py compares every field of the plans (wmdbg_dec_attn_plan / wmdbg_dec_gemv_plan) with it.

Every argument is an int64 numpy array (or a scalar that broadcasts): a function evaluates a whole table of cases at once.
An `if` of the C++ is an np.where over the table; a WM_REQUIRE is a term of `rej`.  The result is a dict of columns named as
the hooks' outputs are; a refused case has rc = WM_ERR_INVALID and every other column 0."""
import numpy as np

WM_OK, WM_ERR_INVALID = 0, 1
WM_DEC_MAXB, ATT_MAXK, WM_MAX_BEST_OF, WM_MAX_TEACHER_PANEL = 128, 1536, 8, 8
DE_QKV, DE_Q, DE_RESID, DE_GELU, DE_LOGITS, DE_LOGITS_X, DE_LOGITS_XR, DE_QKV_P = range(8)
# DecAttnVariant
STREAM, FLAT, FLAT_DEEP_C, FLAT_DEEP_NT, SELF, SELF_OFF, SELF_PANEL, CAND, CAND_FLAT, FQ = range(10)

# struct WmTuning: the fields the launchers read, with the product's values
TUNING = dict(gemv_tn=0, gemv_nblk=0, gemv_ppw2_nblk=0, gemv_no_ppw2=0, prefetch_max_b=16, xattn_split_below=96, xattn_wgs=256,
              xattn_no_flat=0, xattn_lds_pad=84 * 1024, logits_tn=0, xattn_no_deep=0, xattn_fuse_q=1)

ATTN_COLS = ("rc", "variant", "spw", "grid_x", "grid_y", "block", "lds", "n_wg", "warm_tiles", "tile_bytes", "packA", "packB",
             "packC", "combine_grid")
GEMV_COLS = ("rc", "nw", "spw", "tn", "nblk", "ppw", "row_split", "bgroups", "n_tiles", "n_tg", "n_tg_pad", "grid", "block", "lds",
             "pf_tiles", "pf_tile_bytes", "pf_head_major")


def _i(x):
    return np.asarray(x, dtype=np.int64)


def _b(x):
    return np.asarray(x, dtype=bool)


def _cdiv(a, b):
    return (a + b - 1) // b


def _finish(cols, rej, **out):
    shape = np.broadcast(rej, *out.values()).shape
    rej = np.broadcast_to(rej, shape)
    res = {"rc": np.where(rej, WM_ERR_INVALID, WM_OK)}
    for c in cols[1:]:
        res[c] = np.where(rej, 0, np.broadcast_to(_i(out.get(c, 0)), shape))
    return res


def is_x(epi):
    return (epi == DE_LOGITS_X) | (epi == DE_LOGITS_XR)


def is_logits(epi):
    return (epi == DE_LOGITS) | is_x(epi)


def is_qkv(epi):
    return (epi == DE_QKV) | (epi == DE_QKV_P)


def gemv_split(K):
    """wm_dec_gemv_split, one K: (waves, k-steps per wave); (0, 0): no split"""
    steps = K // 32
    for nw in range(16 if steps >= 96 else 8, 0, -1):
        if steps % nw:
            continue
        s = steps // nw
        if s in (2, 4, 5, 6, 8, 10, 12):
            return nw, s
    return 0, 0


def gemv_split_v(K):
    K = _i(K)
    nw, spw = np.zeros_like(K), np.zeros_like(K)
    for k in np.unique(K):
        nw[K == k], spw[K == k] = gemv_split(int(k))
    return nw, spw


def pf_enabled(B, t):
    return B <= t["prefetch_max_b"]


def attn_splits(B, H, t):
    """wm_dec_attn_splits"""
    bh = _i(B) * H
    ns = np.full(bh.shape, 2, dtype=np.int64)
    for _ in range(2):   # while (ns < 8 && bh * ns < 192) ns *= 2
        ns = np.where((ns < 8) & (bh * ns < 192), ns * 2, ns)
    return np.where(bh >= t["xattn_split_below"], 1, ns)


def fq_applies(B, H, K, short_lived, t):
    """wm_dec_xattn_fq_applies"""
    B, H, K, short_lived = _i(B), _i(H), _i(K), _b(short_lived)
    pairs = B * H
    nw, spw = gemv_split_v(np.broadcast_to(K, np.broadcast(B, H, K).shape))
    ok = _b(t["xattn_fuse_q"] != 0) & ~short_lived
    ok = ok & ~((pairs < t["xattn_split_below"]) | (pairs > 256) | (K != H * 64))
    return ok & (nw >= 1) & (nw <= 8) & np.isin(spw, (2, 4, 5, 6))


def _persistent(n_wg, n_cus, short_lived, t):
    n_cus = _i(n_cus)
    cap_cus = np.where((t["xattn_wgs"] > 0) & (t["xattn_wgs"] < n_cus), t["xattn_wgs"], n_cus)
    cap = np.where(short_lived, 1 << 30, cap_cus)
    rounds = _cdiv(n_wg, cap)
    return np.where(n_wg > cap, _cdiv(n_wg, np.maximum(rounds, 1)), n_wg)


def attention(B, H, T_stride, n_keys, nsplit, has_part, has_pf, pf_rows, pf_k, short_lived, n_cus, t):
    """wm_dec_attention"""
    B, H, T_stride, n_keys, nsplit, pf_rows, pf_k, n_cus = map(_i, (B, H, T_stride, n_keys, nsplit, pf_rows, pf_k, n_cus))
    has_part, has_pf, short_lived = map(_b, (has_part, has_pf, short_lived))
    rej = ~np.isin(nsplit, (1, 2, 4, 8))
    rej = rej | ~((T_stride <= ATT_MAXK) & (n_keys <= ATT_MAXK))
    rej = rej | ~((nsplit == 1) | has_part)
    rej = rej | ~((H >= 1) & (H <= 255) & (B * H < 65536))
    n_wg = _persistent(B * H, n_cus, short_lived, t)
    gx = n_wg
    warm = pf_enabled(B, t) & has_pf & (nsplit == 1) & (gx % 8 == 0) & (pf_rows >= 16)
    tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    gx = np.where(warm, gx + pf_rows // 16, gx)
    flat = (nsplit > 1) & _b(t["xattn_no_flat"] == 0)
    pB = T_stride | (n_keys << 16)
    # flat
    units = B * H * 8
    wpw = np.clip(_cdiv(units, 256), 1, 4)
    g = _cdiv(units, wpw)
    rej = rej | (flat & ~(g < 65536))
    deep = np.where(B * H * T_stride * 64 * 2 * 2 <= 3200 * 1024, FLAT_DEEP_C, FLAT_DEEP_NT)
    v_flat = deep if not t["xattn_no_deep"] else FLAT
    ns1 = np.maximum(nsplit, 1)
    return _finish(ATTN_COLS, rej,
                   variant=np.where(flat, v_flat, STREAM),
                   grid_x=np.where(flat, g, gx), grid_y=np.where(flat, 1, nsplit),
                   block=np.where(flat, wpw * 64, (8 // ns1) * 64),
                   lds=np.where(flat, 0, np.where(nsplit == 1, t["xattn_lds_pad"], 0)),
                   n_wg=np.where(flat, g, n_wg),
                   warm_tiles=np.where(flat, 0, gx - n_wg), tile_bytes=np.where(flat, 0, tile_bytes),
                   packA=np.where(flat, H | (8 << 8) | (wpw << 16), H | (nsplit << 8)), packB=pB,
                   packC=np.where(flat, (B * H) | (g << 16), (B * H) | (n_wg << 16)),
                   combine_grid=np.where(nsplit > 1, B * H, 0))


def attention_cand(C, N, H, T_stride, n_keys, has_part, has_pf, pf_rows, pf_k, short_lived, n_cus, t):
    """wm_dec_attention_cand and its launch_xcand"""
    C, N, H, T_stride, n_keys, pf_rows, pf_k, n_cus = map(_i, (C, N, H, T_stride, n_keys, pf_rows, pf_k, n_cus))
    has_part, has_pf, short_lived = map(_b, (has_part, has_pf, short_lived))
    rej = ~((N >= 1) & (N <= WM_MAX_BEST_OF) & (C >= 1) & (C * N <= WM_DEC_MAXB))
    rej = rej | ~((T_stride >= 1) & (T_stride <= ATT_MAXK) & (n_keys >= 1) & (n_keys <= T_stride))
    rej = rej | ~((H >= 1) & (H <= 255))
    rej = rej | ~(has_part | (C * H >= 256) | short_lived)
    pairs = C * H
    flat = (pairs < 256) & ~short_lived
    pB = T_stride | (n_keys << 16)
    pf = pf_enabled(C * N, t) & has_pf & (pf_rows >= 16)
    tile_bytes = np.where(pf, 16 * pf_k * 2, 0)
    warm = np.where(pf, pf_rows // 16, 0)
    # flat
    units = pairs * 8
    wpw = np.clip(_cdiv(units, 256), 1, 8)
    g = _cdiv(units, wpw)
    warm_f = np.where(g % 8 != 0, 0, warm)
    # one workgroup per pair
    n_wg = _persistent(pairs, n_cus, short_lived, t)
    warm_p = np.where(n_wg % 8 != 0, 0, warm)
    rej = rej | (~flat & ~(n_wg < 65536))
    warm = np.where(flat, warm_f, warm_p)
    n = np.where(flat, g, n_wg)
    return _finish(ATTN_COLS, rej, variant=np.where(flat, CAND_FLAT, CAND), grid_x=n + warm, grid_y=1,
                   block=np.where(flat, wpw * 64, 512), n_wg=n, warm_tiles=warm, tile_bytes=np.where(warm > 0, tile_bytes, 0),
                   packA=np.where(flat, H | (wpw << 16), H), packB=pB, packC=C | (n << 16),
                   combine_grid=np.where(flat, C * N * H, 0))


def xattn_fq(B, H, T_stride, n_keys, K, has_pf, pf_rows, pf_k, t):
    """wm_dec_xattn_fq (qa: a LayerNorm-folded K x K query projection)"""
    B, H, T_stride, n_keys, K, pf_rows, pf_k = map(_i, (B, H, T_stride, n_keys, K, pf_rows, pf_k))
    has_pf = _b(has_pf)
    rej = ~(K == H * 64)
    rej = rej | ~((H >= 1) & (H <= 255) & (B >= 1) & (B <= WM_DEC_MAXB) & (T_stride <= ATT_MAXK) & (n_keys >= 1) & (n_keys <= ATT_MAXK))
    nw, spw = gemv_split_v(K)
    rej = rej | ~((nw >= 1) & (nw <= 8))
    grid = 8 * _cdiv(H * B, 8)
    n_wg = grid
    warm = pf_enabled(B, t) & has_pf & (pf_rows >= 16)
    tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    grid = np.where(warm, grid + pf_rows // 16, grid)
    lds = (nw * 1024 + 128 + 64) * 4
    rej = rej | ~np.isin(spw, (2, 4, 5, 6))
    return _finish(ATTN_COLS, rej, variant=FQ, spw=spw, grid_x=grid, grid_y=1, block=512, lds=lds, n_wg=n_wg, warm_tiles=grid - n_wg,
                   tile_bytes=tile_bytes, packA=H | (B << 8), packB=T_stride | (n_keys << 16))


def self_attention(B, H, T_stride, n_keys, has_pos, has_off, has_pf, pf_rows, pf_k, t):
    """wm_dec_self_attention"""
    B, H, T_stride, n_keys, pf_rows, pf_k = map(_i, (B, H, T_stride, n_keys, pf_rows, pf_k))
    has_pos, has_off, has_pf = map(_b, (has_pos, has_off, has_pf))
    rej = ~((T_stride <= ATT_MAXK) & (n_keys <= ATT_MAXK) & (has_pos | (n_keys >= 1)))
    rej = rej | ~((H >= 1) & (H <= 255) & (B * H < 65536))
    gx = B * H
    warm = pf_enabled(B, t) & has_pf & (gx % 8 == 0) & (pf_rows >= 16)
    tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    gx = np.where(warm, gx + pf_rows // 16, gx)
    return _finish(ATTN_COLS, rej, variant=np.where(has_off, SELF_OFF, SELF), grid_x=gx, grid_y=1, block=256, n_wg=B * H,
                   warm_tiles=gx - B * H, tile_bytes=tile_bytes, packA=H | (1 << 8), packB=T_stride | (n_keys << 16),
                   packC=(B * H) | ((B * H) << 16))


def self_attention_panel(C, w, H, T_stride, has_pos, has_pf, pf_rows, pf_k, t):
    """wm_dec_self_attention_panel"""
    C, w, H, T_stride, pf_rows, pf_k = map(_i, (C, w, H, T_stride, pf_rows, pf_k))
    has_pos, has_pf = map(_b, (has_pos, has_pf))
    rej = ~((w >= 1) & (w <= WM_MAX_TEACHER_PANEL) & (C >= 1) & (C * w <= WM_DEC_MAXB))
    rej = rej | ~((T_stride >= w) & (T_stride <= ATT_MAXK) & has_pos)
    rej = rej | ~((H >= 1) & (H <= 255))
    B = C * w
    gx = B * H
    warm = pf_enabled(B, t) & has_pf & (gx % 8 == 0) & (pf_rows >= 16)
    tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    gx = np.where(warm, gx + pf_rows // 16, gx)
    return _finish(ATTN_COLS, rej, variant=SELF_PANEL, grid_x=gx, grid_y=1, block=256, n_wg=B * H, warm_tiles=gx - B * H,
                   tile_bytes=tile_bytes, packA=H | (1 << 8), packB=T_stride, packC=(B * H) | ((B * H) << 16))


def pick_shape(epi, ln, spw, nw, B, n_tiles, n_cus, t):
    """pick_shape: (tn, nblk)"""
    env_tn, env_nb = t["gemv_tn"], t["gemv_nblk"]
    blocks = _cdiv(B, 16)
    one = (blocks < 2) & is_logits(epi) & ln & (spw <= 6)            # -> tn = logits_tn or 4, nblk = 1
    tn_one = t["logits_tn"] if t["logits_tn"] in (1, 2) else 4
    plain = ~one & ((blocks < 2) | (nw > 8) | (spw > 8))             # -> (1, 1)
    nblk = 1 if env_nb == 1 else 2
    wide = ln & (is_qkv(epi) | (epi == DE_GELU) | is_logits(epi)) & (nblk == 2) & (spw <= 6)
    g = _cdiv(blocks, 2)
    best, best_rounds, best_wgs = np.ones_like(g), np.full(g.shape, 1 << 30), np.zeros_like(g)
    for tw in (1, 2, 4):
        wgs = _cdiv(n_tiles, tw) * g
        cap = n_cus * (2 if tw == 1 else 1)
        rounds = _cdiv(wgs, cap)
        fill = n_cus * 3 // 4
        better = (rounds < best_rounds) | ((rounds == best_rounds) & (best_wgs >= fill) & (wgs >= fill))
        best = np.where(better, tw, best)
        best_rounds = np.where(better, rounds, best_rounds)
        best_wgs = np.where(better, wgs, best_wgs)
    if env_tn in (1, 2, 4):
        best = np.full_like(best, env_tn)
    tn = np.where(one, tn_one, np.where(plain | ~wide, 1, best))
    return tn, np.where(one | plain, 1, nblk)


def gemv(epi, ln, B, N, K, has_pf, pf_rows, pf_k, pf_head_major, n_cus, t):
    """wm_dec_gemv and its launch_gemv_shape, for an (epilogue, LayerNorm) pair the GEMV is built for"""
    epi, B, N, K, pf_rows, pf_k, pf_head_major, n_cus = map(_i, (epi, B, N, K, pf_rows, pf_k, pf_head_major, n_cus))
    ln, has_pf = _b(ln), _b(has_pf)
    rej = ~((B >= 1) & (B <= WM_DEC_MAXB))
    rej = rej | ~(K % 32 == 0)
    nw, spw = gemv_split_v(np.broadcast_to(K, np.broadcast(epi, ln, B, N, K, n_cus).shape))
    rej = rej | ~(nw >= 1)
    rej = rej | ~(~ln | ((K % 64 == 0) & (K // 16 <= 80)))
    n_tiles = _cdiv(N, 16)
    tn, nblk = pick_shape(epi, ln, spw, nw, B, n_tiles, n_cus, t)
    bgroups = _cdiv(_cdiv(B, 16), nblk)
    no_ppw = t["gemv_no_ppw2"] != 0
    ppw2 = _b(not no_ppw) & ~ln & (epi == DE_RESID) & (nw == 16) & (B > 16) & (spw >= 6) & (spw <= 10) & (tn == 1) & (nblk == 1)
    ppw = np.where(ppw2, 2, 1)
    blocks = _cdiv(B, 16)
    knob = t["gemv_ppw2_nblk"]
    two = (n_tiles * blocks > n_cus) & (n_tiles * _cdiv(blocks, 2) <= n_cus) if not knob else np.full(ppw2.shape, knob == 2)
    nblk = np.where(ppw2 & two, 2, nblk)
    bgroups = np.where(ppw2 & two, _cdiv(blocks, 2), bgroups)
    n_tg = _cdiv(n_tiles, tn)
    n_tg_pad = np.where(bgroups > 1, _cdiv(n_tg, 8) * 8, n_tg)
    grid = n_tg_pad * bgroups
    warm = pf_enabled(B, t) & has_pf & (pf_rows >= 16) & (grid % 8 == 0)
    pf_tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    pf_tiles = np.where(warm, pf_rows // 16, 0)
    hm = np.where(warm, pf_head_major, 0)
    grid = np.where(warm, grid + np.where(pf_head_major != 0, 32 * (pf_head_major // np.maximum(B, 1) + 2), pf_tiles), grid)
    # launch_gemv: the k-steps per wave the kernels are instantiated for
    rej = rej | ~np.isin(spw, (2, 4, 5, 6, 8, 10, 12))
    # launch_gemv_shape<SPW, EPI, LN>
    resid = ~ln & (epi == DE_RESID)
    TWO = resid & (spw >= 6) & (spw <= 10)
    rej = rej | (ppw2 & ~(TWO & (tn == 1) & (nblk >= 1) & (nblk <= 2) & (nw % 2 == 0)))
    w2 = nw // 2
    lds2 = nw * nblk * 1024 + w2 * 32 * 4
    rej = rej | (ppw2 & (nblk == 2) & (w2 != 8))
    rs2 = (nblk == 2) | ((w2 >= 4) & (B > 1))           # the <.., 2, 4> instantiations
    split = ~ppw2 & resid & (B > 1) & (tn == 1) & (nblk * 4 <= nw)
    ldsr = nw * nblk * 1024 + nw * 32 * 4
    rej = rej | (split & ~((nblk == 1) | ((nblk == 2) & (spw <= 8))))
    lds = nw * tn * nblk * 1024 + nw * 32 * 4
    LOGITS = is_logits(epi)
    WIDE = ln & (is_qkv(epi) | (epi == DE_GELU) | LOGITS) & (spw <= 6)
    have = ((tn == 1) & (nblk == 1)) | ((tn == 1) & (nblk == 2) & (spw <= 8)) | ((tn == 2) & (nblk == 1) & WIDE & LOGITS) | \
           ((tn == 4) & (nblk == 1) & WIDE & LOGITS) | ((tn == 2) & (nblk == 2) & WIDE) | ((tn == 4) & (nblk == 2) & WIDE)
    rej = rej | (~ppw2 & ~split & ~have)
    return _finish(GEMV_COLS, rej, nw=nw, spw=spw, tn=tn, nblk=nblk, ppw=ppw, row_split=np.where(ppw2, rs2, split), bgroups=bgroups,
                   n_tiles=n_tiles, n_tg=n_tg, n_tg_pad=n_tg_pad, grid=grid, block=np.where(ppw2, w2 * 64, nw * 64),
                   lds=np.where(ppw2, lds2, np.where(split, ldsr, lds)), pf_tiles=pf_tiles, pf_tile_bytes=pf_tile_bytes, pf_head_major=hm)
