// dec_launch.cpp -- the decode step's launch plans (dec_launch.h): pure integer arithmetic, no HIP, no context, no globals.
#include "dec_launch.h"

#include <stddef.h>
#include <string.h>

#include "../../include/whisper_mi355x.h"

void wm_set_error(const char *fmt, ...);   // api.cpp (wm_internal.h declares it next to the HIP plumbing)

#define PLAN_REQUIRE(cond, ...)           \
    do {                                  \
        if (!(cond)) {                    \
            wm_set_error(__VA_ARGS__);    \
            return WM_ERR_INVALID;        \
        }                                 \
    } while (0)

// ------------------------------------------------------------------ packed words ----
namespace {
inline bool fits(int v, int bits) { return v >= 0 && (bits >= 31 || v < (1 << bits)); }
}  // namespace

bool wm_pack_attn_keys(int T_stride, int n_keys, unsigned *b) {
    *b = (unsigned)T_stride | ((unsigned)n_keys << 16);
    return fits(T_stride, 16) && fits(n_keys, 16);
}
void wm_unpack_attn_keys(unsigned b, int *T_stride, int *n_keys) {
    *T_stride = (int)(b & 0xffffu);
    *n_keys = (int)(b >> 16);
}
bool wm_pack_attn_rows(int H, int nsplit, int flat_wpw, int n_bh, int n_wg, unsigned *a, unsigned *c) {
    *a = (unsigned)H | ((unsigned)nsplit << 8) | ((unsigned)flat_wpw << 16);
    *c = (unsigned)n_bh | ((unsigned)n_wg << 16);
    return fits(H, 8) && fits(nsplit, 8) && fits(flat_wpw, 16) && fits(n_bh, 16) && fits(n_wg, 16);
}
void wm_unpack_attn_rows(unsigned a, unsigned c, int *H, int *nsplit, int *flat_wpw, int *n_bh, int *n_wg) {
    *H = (int)(a & 0xffu);
    *nsplit = (int)((a >> 8) & 0xffu);
    *flat_wpw = (int)(a >> 16);
    *n_bh = (int)(c & 0xffffu);
    *n_wg = (int)(c >> 16);
}
bool wm_pack_attn_cand(int H, int flat_wpw, int C, int n_wg, unsigned *a, unsigned *c) {
    *a = (unsigned)H | ((unsigned)flat_wpw << 16);
    *c = (unsigned)C | ((unsigned)n_wg << 16);
    return fits(H, 8) && fits(flat_wpw, 16) && fits(C, 16) && fits(n_wg, 16);
}
void wm_unpack_attn_cand(unsigned a, unsigned c, int *H, int *flat_wpw, int *C, int *n_wg) {
    *H = (int)(a & 0xffu);
    *flat_wpw = (int)(a >> 16);
    *C = (int)(c & 0xffffu);
    *n_wg = (int)(c >> 16);
}
bool wm_pack_attn_fq(int H, int B, unsigned *a) {
    *a = (unsigned)H | ((unsigned)B << 8);
    return fits(H, 8) && fits(B, 24);
}
void wm_unpack_attn_fq(unsigned a, int *H, int *B) {
    *H = (int)(a & 0xffu);
    *B = (int)(a >> 8);
}

// ------------------------------------------------------------------ shared rules ----
int wm_dec_warm_tiles(int rows, bool has_pf, int pf_rows, int pf_k, int compute_grid, const WmTuning &t, long *tile_bytes) {
    *tile_bytes = 0;
    if (!(rows <= t.prefetch_max_b && has_pf && pf_rows >= 16 && compute_grid % 8 == 0)) return 0;
    *tile_bytes = 16L * pf_k * 2;
    return pf_rows / 16;
}

int wm_dec_persistent_wgs(int pairs, int n_cus, bool short_lived, const WmTuning &t) {
    // (a sub-chip lane: one persistent workgroup per CU of ITS part of the chip)
    const int cap_cus = t.xattn_wgs > 0 && t.xattn_wgs < n_cus ? t.xattn_wgs : n_cus;
    const int cap = short_lived ? (1 << 30) : cap_cus;
    int n_wg = pairs;
    if (n_wg > cap) {
        const int rounds = (n_wg + cap - 1) / cap;
        n_wg = (n_wg + rounds - 1) / rounds;  // balanced: every workgroup walks `rounds` (or rounds - 1) pairs
    }
    return n_wg;
}

void wm_dec_flat_deal(int pairs, int wave_cap, int *wpw, int *g) {
    const int units = pairs * 8;
    int w = (units + 255) / 256;
    w = w < 1 ? 1 : (w > wave_cap ? wave_cap : w);
    *wpw = w;
    *g = (units + w - 1) / w;
}

int wm_dec_attn_splits(int B, int H, const WmTuning &t) {
    const int bh = B * H;
    // few pairs: the (pair, stream) units are dealt flat over the chip and merged by a combine launch.  (Measured at
    // B = 8 x 20 heads = 160 pairs: flat 11.5 + combine 3.0 us vs 12.2 us for one 8-wave workgroup per pair -- the kernel
    // is bound by bytes in flight per CU, not by idle CUs -- so the split starts below 96 pairs only.)
    const int thr = t.xattn_split_below;   // 96
    if (bh >= thr) return 1;
    int ns = 2;
    while (ns < 8 && bh * ns < 192) ns *= 2;
    return ns;
}

int wm_dec_gemv_split(int K, int *spw) {
    const int steps = K / 32;
    for (int nw = steps >= 96 ? 16 : 8; nw >= 1; --nw) {
        if (steps % nw) continue;
        const int s = steps / nw;
        if (s == 2 || s == 4 || s == 5 || s == 6 || s == 8 || s == 10 || s == 12) {
            if (spw) *spw = s;
            return nw;
        }
    }
    return 0;
}

bool wm_dec_xattn_fq_applies(int B, int H, int K, bool short_lived, const WmTuning &t) {
    if (!t.xattn_fuse_q || short_lived) return false;
    const int pairs = B * H;
    if (pairs < t.xattn_split_below || pairs > 256 || K != H * 64) return false;
    int spw = 0;
    const int nw = wm_dec_gemv_split(K, &spw);
    return nw >= 1 && nw <= 8 && (spw == 2 || spw == 4 || spw == 5 || spw == 6);
}

// ------------------------------------------------------------------ attention plans ----
int wm_plan_attention(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p) {
    const int B = s.B, H = s.H, nsplit = s.nsplit;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(nsplit == 1 || nsplit == 2 || nsplit == 4 || nsplit == 8, "dec_attention: nsplit %d is not 1, 2, 4 or 8", nsplit);
    PLAN_REQUIRE(s.T_stride <= WM_ATT_MAXK && s.n_keys <= WM_ATT_MAXK, "dec_attention: more than %d keys", WM_ATT_MAXK);
    PLAN_REQUIRE(nsplit == 1 || s.has_part, "dec_attention: split launch without a partials buffer");
    PLAN_REQUIRE(H >= 1 && H <= 255 && (long)B * H < 65536, "dec_attention: %d heads x %d rows do not fit the packed arguments", H, B);
    bool ok = wm_pack_attn_keys(s.T_stride, s.n_keys, &p->w.b);
    if (nsplit > 1 && !t.xattn_no_flat) {
        // few pairs: deal the (pair, stream) units evenly over ~256 workgroups (see the kernel)
        int wpw, g;
        wm_dec_flat_deal(B * H, 4, &wpw, &g);   // < 96 pairs = < 768 units: <= 3 waves
        PLAN_REQUIRE(g < 65536, "dec_attention: flat grid too large");
        // (DEEP: every block of a stream requested up front -- the flat deal is the latency regime by construction)
        ok = wm_pack_attn_rows(H, 8, wpw, B * H, g, &p->w.a, &p->w.c) && ok;
        if (t.xattn_no_deep) p->variant = DAV_FLAT;
        // a cache of <= 3.2 MB per layer (tiny.en / base, single chunk) stays in the L2s from one position to the next
        // when it is read with cacheable loads: -1 .. -2 % per position there; +5 % at `small` (4.6 MB): the rule
        else if ((size_t)B * H * s.T_stride * 64 * 2 * 2 <= (size_t)3200 * 1024) p->variant = DAV_FLAT_DEEP_C;
        else p->variant = DAV_FLAT_DEEP_NT;
        p->n_wg = p->grid_x = g;
        p->grid_y = 1;
        p->block = wpw * 64;
    } else {
        // 8 streams x 4 loads = 126 VGPRs: an 8-wave GEMV workgroup of another decode group fits beside one of these on a
        // CU (a second cross-attention workgroup does not: LDS reservation below); at most 256 workgroups -- one per CU --
        // walk the pairs, balanced (56 chunks x 20 heads = 224 workgroups x 5 pairs).  Measured alone at B = 8 / 56 / 128:
        // 12.8 / 67 / 144 us (4.8 / 6.4 / 6.8 TB/s: ~6.4 is what HBM reads deliver).
        // short_lived (the chip is shared with other decode groups): one workgroup per pair, see WmModel::xattn_shared
        const int n_wg = wm_dec_persistent_wgs(B * H, n_cus, s.short_lived, t);
        p->warm_tiles = wm_dec_warm_tiles(B, s.has_pf && nsplit == 1, s.pf_rows, s.pf_k, n_wg, t, &p->tile_bytes);
        ok = wm_pack_attn_rows(H, nsplit, 0, B * H, n_wg, &p->w.a, &p->w.c) && ok;
        p->variant = DAV_STREAM;
        p->n_wg = n_wg;
        p->grid_x = n_wg + p->warm_tiles;
        p->grid_y = nsplit;
        p->block = (8 / nsplit) * 64;
        // ONE cross-attention workgroup per CU, chip-wide: a workgroup reserves more than half of the CU's 160 KB of
        // LDS (it uses 2 KB), so the cross-attention launches of the decode groups in flight take the CUs one after
        // the other instead of side by side.  A single launch already saturates the HBM (6.4 TB/s alone); a second
        // one beside it adds no bandwidth but fills the SIMDs' wave slots / VGPRs for the whole launch (persistent
        // workgroups), and the other groups' GEMVs -- which fit beside ONE such workgroup, LDS included (<= 66 KB) --
        // wait.  Measured, 3 groups in flight: 1920 -> 1966 audio-s/s (20 steps), 2014 -> 2118 (72 steps, decode stage
        // 0.74 -> 0.79 of the HBM peak).
        p->lds = nsplit == 1 ? t.xattn_lds_pad : 0;   // 84 KB
    }
    PLAN_REQUIRE(ok, "dec_attention: a packed argument does not fit its bits");
    p->combine_grid = nsplit > 1 ? B * H : 0;
    return WM_OK;
}

int wm_plan_attention_cand(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p) {
    const int C = s.C, N = s.N, H = s.H;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(N >= 1 && N <= WM_MAX_BEST_OF && C >= 1 && (long)C * N <= WM_DEC_MAXB,
                 "dec_attention_cand: %d windows x %d candidates outside 1 .. %d rows of 1 .. %d candidates", C, N, WM_DEC_MAXB,
                 WM_MAX_BEST_OF);
    PLAN_REQUIRE(s.T_stride >= 1 && s.T_stride <= WM_ATT_MAXK && s.n_keys >= 1 && s.n_keys <= s.T_stride,
                 "dec_attention_cand: 1 .. %d keys", WM_ATT_MAXK);
    PLAN_REQUIRE(H >= 1 && H <= 255, "dec_attention_cand: %d heads do not fit the packed arguments", H);
    PLAN_REQUIRE(s.has_part || C * H >= 256 || s.short_lived, "dec_attention_cand: flat launch without a partials buffer");
    const int pairs = C * H;
    const bool flat = pairs < 256 && !s.short_lived;
    bool ok = wm_pack_attn_keys(s.T_stride, s.n_keys, &p->w.b);
    if (flat) {
        // few pairs (8 windows x 20 heads = 160): every CU streams an equal share of the (pair, stream) units
        int wpw, g;
        wm_dec_flat_deal(pairs, 8, &wpw, &g);
        ok = wm_pack_attn_cand(H, wpw, C, g, &p->w.a, &p->w.c) && ok;
        p->variant = DAV_CAND_FLAT;
        p->n_wg = g;
        p->block = wpw * 64;
        p->combine_grid = C * N * H;
    } else {
        // one 8-wave workgroup per pair, at most one per CU (persistent, balanced), or one per pair when the chip is shared
        const int n_wg = wm_dec_persistent_wgs(pairs, n_cus, s.short_lived, t);
        PLAN_REQUIRE(n_wg < 65536, "dec_attention_cand: grid too large");
        ok = wm_pack_attn_cand(H, 0, C, n_wg, &p->w.a, &p->w.c) && ok;
        p->variant = DAV_CAND;
        p->n_wg = n_wg;
        p->block = 512;
    }
    PLAN_REQUIRE(ok, "dec_attention_cand: a packed argument does not fit its bits");
    // (the warm-up tiles follow the compute workgroups: keep their XCD placement)
    p->warm_tiles = wm_dec_warm_tiles(C * N, s.has_pf, s.pf_rows, s.pf_k, p->n_wg, t, &p->tile_bytes);
    p->grid_x = p->n_wg + p->warm_tiles;
    p->grid_y = 1;
    return WM_OK;
}

int wm_plan_xattn_fq(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p) {
    (void)n_cus;   // 96 .. 256 pairs: one workgroup per pair whatever the lane
    const int B = s.B, H = s.H;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(s.K == (long)H * 64, "xattn_fq: not a LayerNorm-folded d x d query projection");
    PLAN_REQUIRE(H >= 1 && H <= 255 && B >= 1 && B <= WM_DEC_MAXB && s.T_stride <= WM_ATT_MAXK && s.n_keys >= 1 && s.n_keys <= WM_ATT_MAXK,
                 "xattn_fq: bad geometry");
    int spw = 0;
    const int nw = wm_dec_gemv_split(s.K, &spw);
    PLAN_REQUIRE(nw >= 1 && nw <= 8, "xattn_fq: K split over more than 8 waves");
    PLAN_REQUIRE(spw == 2 || spw == 4 || spw == 5 || spw == 6, "xattn_fq: unsupported k-steps per wave %d", spw);
    const bool ok = wm_pack_attn_fq(H, B, &p->w.a) && wm_pack_attn_keys(s.T_stride, s.n_keys, &p->w.b);
    PLAN_REQUIRE(ok, "xattn_fq: a packed argument does not fit its bits");
    p->variant = DAV_FQ;
    p->spw = spw;
    p->n_wg = 8 * ((H * B + 7) / 8);
    p->warm_tiles = wm_dec_warm_tiles(B, s.has_pf, s.pf_rows, s.pf_k, p->n_wg, t, &p->tile_bytes);
    p->grid_x = p->n_wg + p->warm_tiles;
    p->grid_y = 1;
    p->block = 512;
    p->lds = (int)(((size_t)nw * 1024 + 128 + 64) * sizeof(float));
    return WM_OK;
}

int wm_plan_self_attention(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p) {
    (void)n_cus;
    const int B = s.B, H = s.H;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(s.T_stride <= WM_ATT_MAXK && s.n_keys <= WM_ATT_MAXK && (s.has_pos || s.n_keys >= 1), "dec_self_attention: 1..%d keys",
                 WM_ATT_MAXK);
    PLAN_REQUIRE(H >= 1 && H <= 255 && (long)B * H < 65536, "dec_self_attention: %d heads x %d rows do not fit the packed arguments", H, B);
    // a pair is 15-57 KB of cache (<= 448 rows, ~115 on average over a 224-token decode): ONE 4-wave workgroup
    const bool ok = wm_pack_attn_rows(H, 1, 0, B * H, B * H, &p->w.a, &p->w.c) && wm_pack_attn_keys(s.T_stride, s.n_keys, &p->w.b);
    PLAN_REQUIRE(ok, "dec_self_attention: a packed argument does not fit its bits");
    p->variant = s.has_off ? DAV_SELF_OFF : DAV_SELF;   // a ragged decode group: the instantiation that places every pair at its row offset
    p->n_wg = B * H;
    p->warm_tiles = wm_dec_warm_tiles(B, s.has_pf, s.pf_rows, s.pf_k, p->n_wg, t, &p->tile_bytes);
    p->grid_x = p->n_wg + p->warm_tiles;
    p->grid_y = 1;
    p->block = 256;
    return WM_OK;
}

int wm_plan_self_attention_panel(const DecAttnShape &s, int n_cus, const WmTuning &t, DecAttnPlan *p) {
    (void)n_cus;
    const int C = s.C, w = s.N, H = s.H;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(w >= 1 && w <= WM_MAX_TEACHER_PANEL && C >= 1 && (long)C * w <= WM_DEC_MAXB,
                 "dec_self_attention_panel: %d windows x %d positions outside 1 .. %d rows of 1 .. %d positions", C, w, WM_DEC_MAXB,
                 WM_MAX_TEACHER_PANEL);
    PLAN_REQUIRE(s.T_stride >= w && s.T_stride <= WM_ATT_MAXK && s.has_pos, "dec_self_attention_panel: %d .. %d cache rows", w, WM_ATT_MAXK);
    PLAN_REQUIRE(H >= 1 && H <= 255, "dec_self_attention_panel: %d heads do not fit the packed arguments", H);
    const int B = C * w;
    const bool ok = wm_pack_attn_rows(H, 1, 0, B * H, B * H, &p->w.a, &p->w.c) && wm_pack_attn_keys(s.T_stride, 0, &p->w.b);
    PLAN_REQUIRE(ok, "dec_self_attention_panel: a packed argument does not fit its bits");
    p->variant = s.has_off ? DAV_SELF_OFF_PANEL : DAV_SELF_PANEL;   // a ragged group's prompt panel: the same launch shape
    p->n_wg = B * H;
    p->warm_tiles = wm_dec_warm_tiles(B, s.has_pf, s.pf_rows, s.pf_k, p->n_wg, t, &p->tile_bytes);
    p->grid_x = p->n_wg + p->warm_tiles;
    p->grid_y = 1;
    p->block = 256;
    return WM_OK;
}

// ------------------------------------------------------------------ GEMV plan ----
namespace {
// Launch shape at batch B -- tiles per workgroup (TN), batch blocks per workgroup (NBLK) and workgroups per tile group
// (bgroups).  A scheduling choice only: every output element is computed by the same instruction sequence for any shape.
// Small batches (one block): one tile per workgroup, as many workgroups as tiles (latency).  Large batches: two blocks
// per workgroup and, for the wide matrices, 2 or 4 tiles per workgroup so that the grid stays near one round of the chip
// and an activation fragment is fetched once per TN products.
void pick_shape(int epi, bool ln, int spw, int nw, int B, int n_tiles, int n_cus, const WmTuning &t, int *tn, int *nblk) {
    const int env_tn = t.gemv_tn, env_nb = t.gemv_nblk;   // 0 in the product
    const int blocks = (B + 15) / 16;
    *tn = 1;
    *nblk = 1;
    // one block, a 16-wave K split (K = 4d at d >= 768: the multi-unit kernels are built for <= 8 waves -- launch bounds
    // 512, register budget) or more than 8 k-steps per wave (K = 4d at d = 576 / 640: spw 12 / 10 on <= 8 waves -- the
    // two-block kernel holds 2 x SPW activation fragments and exists for SPW <= 8 only): one unit per workgroup, more
    // workgroups along the batch
    if (blocks < 2 && de_is_logits(epi) && ln && spw <= 6) {
        // the vocabulary product of a one-block group: 4 tiles per workgroup (810 workgroups instead of 3 242 two-wave
        // ones; -1.4 % per position at tiny.en / base / small, neutral at large-v2: profiles/r04_latency_probe.txt)
        *tn = (t.logits_tn == 1 || t.logits_tn == 2) ? t.logits_tn : 4;
        return;
    }
    if (blocks < 2 || nw > 8 || spw > 8) return;
    *nblk = env_nb == 1 ? 1 : 2;
    const bool wide = ln && (de_is_qkv(epi) || epi == DE_GELU || de_is_logits(epi)) && *nblk == 2 && spw <= 6;
    if (!wide) return;
    // Tile-group width by RESIDENCY ROUNDS: an 8-wave workgroup of the (1, 2) shape needs <= 128 VGPRs and sits two per
    // CU, the wide shapes (136-190 VGPRs) one per CU; a grid that needs a second round of the chip costs a whole kernel
    // time (measured: fc1 at 56 rows as 320 one-per-CU workgroups = two rounds), so: fewest rounds first, then the
    // narrowest group that still leaves >= 192 workgroups, else the widest.  (Groups of THREE tiles -- fc1 of d = 1280 at
    // 49 .. 64 rows as 214 workgroups of 162 VGPRs instead of 160 of 186 -- were built in round 5 and cost the three-lane
    // run 2 %: 2078 vs 2114-2125 audio-s/s, NOTEBOOK round 5.)
    const int g = (blocks + 1) / 2;
    int best = 1, best_rounds = 1 << 30, best_wgs = 0;
    for (int tw = 1; tw <= 4; tw *= 2) {
        const int wgs = ((n_tiles + tw - 1) / tw) * g;
        const int cap = n_cus * (tw == 1 ? 2 : 1);   // n_cus: 256, or the CUs of a sub-chip lane (wm_ctx::n_cus)
        const int rounds = (wgs + cap - 1) / cap;
        const int fill = n_cus * 3 / 4;              // "still fills the chip": 192 of 256
        const bool better = rounds < best_rounds || (rounds == best_rounds && best_wgs >= fill && wgs >= fill);
        if (better) { best = tw; best_rounds = rounds; best_wgs = wgs; }
    }
    if (env_tn == 1 || env_tn == 2 || env_tn == 4) best = env_tn;
    *tn = best;
}
}  // namespace

int wm_plan_gemv(const DecGemvShape &s, int n_cus, const WmTuning &t, DecGemvPlan *p) {
    const int epi = s.epi, B = s.B;
    const bool ln = s.ln;
    memset(p, 0, sizeof(*p));
    PLAN_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, "dec_gemv: B=%d out of range", B);
    PLAN_REQUIRE(s.K % 32 == 0, "dec_gemv: K=%d must be a multiple of 32", s.K);
    int spw = 0;
    const int nw = wm_dec_gemv_split(s.K, &spw);
    PLAN_REQUIRE(nw >= 1, "dec_gemv: K=%d cannot be split over the waves of a workgroup", s.K);
    PLAN_REQUIRE(!ln || (s.K % 64 == 0 && s.K / 16 <= 80),
                 "dec_gemv: LayerNorm mode needs the producer's K/16 partial statistics (K a multiple of 64, <= 1280)");
    p->nw = nw;
    p->spw = spw;
    p->n_tiles = (s.N + 15) / 16;
    int tn = 1, nblk = 1;
    pick_shape(epi, ln, spw, nw, B, p->n_tiles, n_cus, t, &tn, &nblk);
    p->bgroups = ((B + 15) / 16 + nblk - 1) / nblk;
    // the 16-part K = 4d residual product at more than one batch block: two parts per wave, 8-wave workgroups (two per
    // CU).  pick_shape keeps every 16-wave split at one (tile, block) unit per workgroup, which is what the two-part
    // kernel is built for (d = 768 / 1024 / 1280: spw = 6 / 8 / 10).
    const bool no_ppw = t.gemv_no_ppw2 != 0;
    const int ppw = (!no_ppw && !ln && epi == DE_RESID && nw == 16 && B > 16 && spw >= 6 && spw <= 10 && tn == 1 && nblk == 1) ? 2 : 1;
    if (ppw == 2) {
        // ... and TWO batch blocks per workgroup (a weight fragment feeds two products; 144 VGPRs at spw 10: one workgroup per
        // CU) when the one-block grid would not fit one workgroup per CU but the two-block grid does: 1.25 workgroups per CU
        // run at the pace of the CUs that hold two.  Measured alone, d = 1280: 53 .. 96 rows 12.2 -> 9.9 us, 128 rows (640
        // two-per-CU vs 320 one-per-CU workgroups) 15.5 vs 16.7: the rule; d = 768 / 1024 at 96 / 128 rows: 5.9 -> 5.8 / 8.7 -> 8.1
        // (profiles/r05_fc2_two_blocks.txt).  Same parts, same order of the sums: same bits.
        const int blocks = (B + 15) / 16;
        const int knob = t.gemv_ppw2_nblk;   // probes: 1 / 2 force the shape
        const bool two = knob ? knob == 2 : (p->n_tiles * blocks > n_cus && p->n_tiles * ((blocks + 1) / 2) <= n_cus);
        if (two) {
            nblk = 2;
            p->bgroups = (blocks + 1) / 2;
        }
    }
    p->tn = tn;
    p->nblk = nblk;
    p->ppw = ppw;
    p->n_tg = (p->n_tiles + tn - 1) / tn;
    p->n_tg_pad = p->bgroups > 1 ? (p->n_tg + 7) / 8 * 8 : p->n_tg;  // (tile group, batch group) decode needs rows of 8
    p->grid = p->n_tg_pad * p->bgroups;
    p->pf_tiles = wm_dec_warm_tiles(B, s.has_pf, s.pf_rows, s.pf_k, p->grid, t, &p->pf_tile_bytes);
    if (p->pf_tiles) {
        p->pf_head_major = s.pf_head_major;   // = pairs per XCD of the fused consumer (0: plain placement, tile t on XCD t % 8)
        // head-major: 8 XCDs x 4 tiles x the heads an XCD can host (a range of `per` pairs touches <= per / B + 2 heads)
        p->grid += s.pf_head_major ? 32 * (s.pf_head_major / B + 2) : p->pf_tiles;
    }
    // the kernel of the shape: which instantiations exist (launch_gemv_shape in dec_kernels.hip dispatches to them)
    PLAN_REQUIRE(spw == 2 || spw == 4 || spw == 5 || spw == 6 || spw == 8 || spw == 10 || spw == 12,
                 "dec_gemv: unsupported k-steps per wave %d", spw);
    const bool resid = !ln && epi == DE_RESID;
    if (ppw == 2) {  // 16 K parts on 8 waves (the K = 4d residual products at more than one batch block)
        const bool two = resid && spw >= 6 && spw <= 10;
        PLAN_REQUIRE(two && tn == 1 && nblk >= 1 && nblk <= 2 && nw % 2 == 0, "dec_gemv: no two-part kernel for this shape");
        const int w2 = nw / 2;
        // two batch blocks per workgroup: a weight fragment feeds two products (w2 == 8: four waves per unit)
        PLAN_REQUIRE(nblk != 2 || w2 == 8, "dec_gemv: the two-block two-part kernel needs 8 waves");
        // (row split, see the kernel: four waves per unit finish the residual epilogue; w2 >= 4 and more than one sequence)
        p->row_split = nblk == 2 || (w2 >= 4 && B > 1);
        p->block = w2 * 64;
        p->lds = (long)nw * nblk * 1024 + (long)w2 * 32 * 4;
        return WM_OK;
    }
    p->block = nw * 64;
    if (resid && B > 1 && tn == 1 && nblk * 4 <= nw) {   // four waves per (tile, block) unit
        PLAN_REQUIRE(nblk == 1 || (nblk == 2 && spw <= 8), "dec_gemv: unsupported row-split shape (nblk %d, spw %d)", nblk, spw);
        p->row_split = 1;
        p->lds = (long)nw * nblk * 1024 + (long)nw * 32 * 4;
        return WM_OK;
    }
    const bool logits = de_is_logits(epi);
    const bool wide = ln && (de_is_qkv(epi) || epi == DE_GELU || logits) && spw <= 6;
    const bool have = (tn == 1 && nblk == 1) || (tn == 1 && nblk == 2 && spw <= 8) || ((tn == 2 || tn == 4) && nblk == 1 && wide && logits) ||
                      ((tn == 2 || tn == 4) && nblk == 2 && wide);
    PLAN_REQUIRE(have, "dec_gemv: unsupported launch shape (tn %d, nblk %d, spw %d)", tn, nblk, spw);
    p->lds = (long)nw * tn * nblk * 1024 + (long)nw * 32 * 4;
    return WM_OK;
}

// ------------------------------------------------------------------ flat forms ----
void wm_attn_plan_flat(const int32_t *in, const WmTuning &t, int32_t *out) {
    DecAttnShape s;
    memset(&s, 0, sizeof(s));
    s.B = in[1]; s.C = in[2]; s.N = in[3]; s.H = in[4]; s.T_stride = in[5]; s.n_keys = in[6]; s.nsplit = in[7]; s.K = in[8];
    const int f = in[9];
    s.has_pos = f & 1; s.has_part = f & 2; s.has_off = f & 4; s.has_pf = f & 8; s.short_lived = f & 16;   // (bit 5, the live list: no plan reads it)
    s.pf_rows = in[10]; s.pf_k = in[11];
    const int n_cus = in[12];
    DecAttnPlan p;
    memset(&p, 0, sizeof(p));
    int rc = WM_ERR_INVALID;
    switch (in[0]) {
        case 0: rc = wm_plan_attention(s, n_cus, t, &p); break;
        case 1: rc = wm_plan_attention_cand(s, n_cus, t, &p); break;
        case 2: rc = wm_plan_xattn_fq(s, n_cus, t, &p); break;
        case 3: rc = wm_plan_self_attention(s, n_cus, t, &p); break;
        case 4: rc = wm_plan_self_attention_panel(s, n_cus, t, &p); break;
        default: wm_set_error("attention plan: unknown form %d", in[0]);
    }
    memset(out, 0, sizeof(int32_t) * WM_ATTN_PLAN_OUT);
    out[0] = rc;
    // the two rules the decode step asks before it plans: the cross-attention's split count, the fused launch's test
    const bool sane = s.B >= 0 && s.B <= WM_DEC_MAXB && s.H >= 0 && s.H <= 255;
    if (in[0] == 0 && sane) out[14] = wm_dec_attn_splits(s.B, s.H, t);
    if (in[0] == 2 && sane) out[14] = wm_dec_xattn_fq_applies(s.B, s.H, s.K, s.short_lived, t) ? 1 : 0;
    if (rc != WM_OK) return;
    out[1] = p.variant; out[2] = p.spw; out[3] = p.grid_x; out[4] = p.grid_y; out[5] = p.block; out[6] = p.lds; out[7] = p.n_wg;
    out[8] = p.warm_tiles; out[9] = (int32_t)p.tile_bytes; out[10] = (int32_t)p.w.a; out[11] = (int32_t)p.w.b; out[12] = (int32_t)p.w.c;
    out[13] = p.combine_grid;
}

void wm_gemv_plan_flat(const int32_t *in, const WmTuning &t, int32_t *out) {
    DecGemvShape s;
    memset(&s, 0, sizeof(s));
    s.epi = in[0]; s.ln = in[1] != 0; s.B = in[2]; s.N = in[3]; s.K = in[4];
    s.has_pf = in[5] != 0; s.pf_rows = in[6]; s.pf_k = in[7]; s.pf_head_major = in[8];
    DecGemvPlan p;
    const int rc = wm_plan_gemv(s, in[9], t, &p);
    memset(out, 0, sizeof(int32_t) * WM_GEMV_PLAN_OUT);
    out[0] = rc;
    if (rc != WM_OK) return;
    out[1] = p.nw; out[2] = p.spw; out[3] = p.tn; out[4] = p.nblk; out[5] = p.ppw; out[6] = p.row_split; out[7] = p.bgroups;
    out[8] = p.n_tiles; out[9] = p.n_tg; out[10] = p.n_tg_pad; out[11] = p.grid; out[12] = p.block; out[13] = (int32_t)p.lds;
    out[14] = p.pf_tiles; out[15] = (int32_t)p.pf_tile_bytes; out[16] = p.pf_head_major;
}
