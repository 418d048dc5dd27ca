"""Restatement of the prompt-panel arithmetic (wm_set_prompt_panel), in numpy over whole tables of cases:

  plan(G, width, P, sot_pos, acap_base)  -- tx_plan.cpp wm_prompt_panel_plan: P0, the slice cut and the panel steps;
  self_attention_panel_off(...)          -- dec_launch.cpp wm_plan_self_attention_panel with the windows' offsets.

tests/test_prompt_panel_cpu.py compares the host-only hooks wmdbg_prompt_panel_plan_batch / wmdbg_dec_attn_plan with it."""
import numpy as np

WM_OK, WM_ERR_INVALID = 0, 1
WM_DEC_MAXB, ATT_MAXK, MAX_WIDTH = 128, 1536, 8
SELF_PANEL, SELF_OFF_PANEL = 6, 10   # DecAttnVariant
PLAN_COLS = ("P0", "C", "w", "slices", "steps")
ATTN_COLS = ("rc", "variant", "spw", "grid_x", "grid_y", "block", "lds", "n_wg", "warm_tiles", "tile_bytes", "packA", "packB",
             "packC", "combine_grid")


def _i(x):
    return np.asarray(x, dtype=np.int64)


def _cdiv(a, b):
    return (a + b - 1) // b


def p0(P, sot_pos, acap_base):
    """the first position whose logits the call reads"""
    P, sot_pos, acap_base = map(_i, (P, sot_pos, acap_base))
    r = np.where(sot_pos >= 0, sot_pos, P - 1)
    return np.where((acap_base >= 0) & (acap_base < r), acap_base, r)


def slices(G, width, T):
    """the teacher-forced slice rule: among the widths w' <= width, slices of floor(128 / w') windows, the fewest
    slices x ceil(T / w') steps (ties: the wider); balanced slices.  Returns (C, w')."""
    G, width, T = map(_i, (G, width, T))
    best_w = width.copy()
    best_steps = np.full(G.shape, 1 << 30, dtype=np.int64)
    for wc in range(MAX_WIDTH, 0, -1):
        cap = WM_DEC_MAXB // wc
        steps = _cdiv(G, cap) * _cdiv(T, wc)
        take = (wc <= width) & (steps < best_steps)
        best_steps = np.where(take, steps, best_steps)
        best_w = np.where(take, wc, best_w)
    cap = WM_DEC_MAXB // best_w
    n_slices = _cdiv(G, cap)
    return _cdiv(G, n_slices), best_w


def plan(G, width, P, sot_pos, acap_base):
    G, width, P, sot_pos, acap_base = np.broadcast_arrays(*map(_i, (G, width, P, sot_pos, acap_base)))
    first = p0(P, sot_pos, acap_base)
    on = (width > 1) & (first >= 2)
    C, w = slices(G, width, np.maximum(first, 1))
    z = np.zeros_like(first)
    return dict(P0=first, C=np.where(on, C, z), w=np.where(on, w, z), slices=np.where(on, _cdiv(G, C), z),
                steps=np.where(on, _cdiv(first, w), z))


def self_attention_panel_off(C, w, H, T_stride, has_pos, has_off, has_pf, pf_rows, pf_k, prefetch_max_b=16):
    """wm_plan_self_attention_panel: the launch shape of the uniform panel, the ragged instantiation when has_off"""
    C, w, H, T_stride, pf_rows, pf_k = map(_i, (C, w, H, T_stride, pf_rows, pf_k))
    has_pos, has_off, has_pf = (np.asarray(x, dtype=bool) for x in (has_pos, has_off, has_pf))
    rej = ~((w >= 1) & (w <= MAX_WIDTH) & (C >= 1) & (C * w <= WM_DEC_MAXB))
    rej = rej | ~((T_stride >= w) & (T_stride <= ATT_MAXK) & has_pos)
    rej = rej | ~((H >= 1) & (H <= 255))
    B = C * w
    gx = B * H
    warm = (B <= prefetch_max_b) & has_pf & (gx % 8 == 0) & (pf_rows >= 16)
    tile_bytes = np.where(warm, 16 * pf_k * 2, 0)
    gx = np.where(warm, gx + pf_rows // 16, gx)
    out = dict(variant=np.where(has_off, SELF_OFF_PANEL, SELF_PANEL), grid_x=gx, grid_y=1, block=256, n_wg=B * H,
               warm_tiles=gx - B * H, tile_bytes=tile_bytes, packA=H | (1 << 8), packB=T_stride, packC=(B * H) | ((B * H) << 16))
    shape = np.broadcast(rej, *out.values()).shape
    rej = np.broadcast_to(rej, shape)
    res = {"rc": np.where(rej, WM_ERR_INVALID, WM_OK)}
    for c in ATTN_COLS[1:]:
        res[c] = np.where(rej, 0, np.broadcast_to(_i(out.get(c, 0)), shape))
    return res
