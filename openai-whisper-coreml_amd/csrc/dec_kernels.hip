// dec_kernels.hip -- the autoregressive decode step for gfx950 (SURVEY.md section 2 rows
// K10-K14): one decoder position for a decode GROUP of 1 .. 128 sequences with KV caches.
//
// Regime: every matrix product is a skinny GEMM that streams each weight exactly once per group and position --
// HBM-bound, and at Whisper's sizes latency-bound per launch.  Design (details at each kernel):
//   * dec_gemv_kernel: a workgroup owns TN adjacent 16-row weight tiles and NBLK blocks of 16 batch rows (the batch is
//     the M of v_mfma_f32_16x16x32_bf16); its waves split K by a rule that depends on K ONLY (bit-level batch
//     invariance); weights are stored fragment-tiled (one coalesced dwordx4 per lane per k-step, straight into VGPRs),
//     activations likewise; everything is requested up front (one memory round trip); LayerNorm is FOLDED into the
//     weights (W' = W gamma) with the row statistics arriving as deterministic partial sums from the producer of the
//     residual; bias, GELU, residual add (+ bf16 copy + next statistics), KV-cache append and the logits arg-max with the
//     suppress bitmaps / timestamp rules are fused epilogues, so a decoder layer is 8 launches.  Round 5: the scalars a
//     kernel's first loads need are LEADING scalar arguments, preloaded into SGPRs (no kernel-argument fetch in front of
//     the first weight load: tests/test_isa_cpu.py); the residual epilogue is finished by four waves per unit.
//   * dec_xrows_attn_kernel (cross, streaming / flat) and dec_rows_attn_kernel (self; flat deep cross): single-query
//     attention over a bf16 K/V cache as NS canonical row streams per (sequence, head) pair (8 cross, 4 self), 8 lanes per
//     128-byte row, fp32 online softmax per stream, one ordered merge -- the same arithmetic whatever the launch shape.
//     With early stop on they walk the compact list of LIVE rows.
//   * dec_xattn_fq_kernel: cross_attn_ln + query projection INSIDE the cross-attention launch for 96 .. 256 pairs alone on
//     the device (7 launches per layer), bit-identical to the two launches.  The three attention kernels have their own
//     prologue, loop driver and query load; a stream's block loads, block arithmetic and row-group reduction are written
//     once (attn_load_block, attn_block, attn_stream_reduce), and so is the merge (attn_merge_core).
//   * argmax_embed_kernel: closes a position (arg-max reduce, timestamp decision, early-stop flags + live list, next
//     token, next embedding + statistics) and advances the decode position, which lives in HBM (*pos_ptr) -- so ONE
//     captured hipGraph of the whole position (and one of WM_BURST positions) replays for every position.
#include <stdlib.h>

#include <atomic>
#include <string.h>

#include "dec_close.h"
#include "model.h"
#include "philox.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

__device__ __forceinline__ unsigned pack2(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
struct DecGemvDev {
    int B, N, K;
    const bf16_t *W;        // WL_TILED [N padded to 16][K]; LayerNorm modes: gamma folded in (W_nk * g_k, rounded to bf16)
    const float *c1;        // LayerNorm fold: c1[n] = sum_k W'_nk (the folded, rounded weights); plain modes: unused
    const float *c2;        // bias[n] (+ sum_k beta_k W_nk in LayerNorm modes); may be null
    const bf16_t *a;        // [B][K] bf16 activations: bf16 copy of the residual, attention output or GELU output
    const float *stats_in;  // LayerNorm: [blk][stats_parts][16][2] partial (sum x, sum x^2) per row of the f32 residual
    int stats_parts;
    long stats_stride;      // floats between the statistics of consecutive 16-row batch blocks
    float *stats_out;       // DE_RESID: this launch's per-tile partials of the UPDATED residual
    // The bf16 copy of the residual is stored MEAN-CENTRED: xb = bf16(x - off_b), off_b = the row's LayerNorm mean as of
    // the previous LayerNorm (mean_in).  bf16 rounding then scales with |x - mean| (as it did when the normalised row was
    // rounded), not with |x|: a common-mode offset of the stream -- which LayerNorm removes -- would otherwise cost
    // 2^-9 |offset| per element (measured: offset 1.0 at std 0.2 -> logits rel-L2 4.6e-2; 10.0 -> 0.43).  The LayerNorm-
    // folded GEMV reads the same offset, uses (mean - off) in the fold and leaves the new mean in mean_out (the other
    // buffer of a ping-pong pair, so no workgroup of the launch can see it).  Null: offset 0 / nothing written.
    const float *mean_in;
    float *mean_out;
    float *out_f32;
    bf16_t *out_bf16;
    bf16_t *kcache, *vcache;
    const int *pos_ptr;  // decode position lives in HBM so a captured hipGraph replays unchanged
    int n_ctx, n_head;
    long ldo;
    unsigned long long *tilemax;  // [B][n_tiles] (DE_LOGITS)
    int n_tiles;                  // 16-row weight tiles
    int n_tg, n_tg_pad;           // tile groups (TN tiles each); n_tg_pad: rounded up to 8 when a group is shared by several workgroups
    int arg_first, arg_last;
    const unsigned *mask;  // DE_LOGITS: suppressed-token bitmaps [2][mask_words] or null
    int mask_words, mask_first_pos;
    WmTsDev ts;            // DE_LOGITS: timestamp rules (ts.rng == null: off)
    WmXDev x;              // DE_LOGITS_X: extended decode (read in the epilogue only)
    const char *pf_ptr;    // next GEMV's weights: extra workgroups pull them into this XCD's L2
    long pf_tile_bytes;    // bytes of one 16-row weight tile of that matrix
    int pf_tiles;
    int pf_head_major;     // warm-up placement for a consumer that runs head h on XCD h % 8 (dec_xattn_fq_kernel)
    int bgroups;           // workgroups per tile group along the batch: group g takes batch rows [g, g + 1) * NBLK * 16
    WmRepDev rep;          // DE_LOGITS_XR: repetition rules (behind the older fields: they keep their kernel-argument offsets)
    int panel;             // DE_QKV_P: panel width (cold, like rep: read in the epilogue only)
    WmSbEpi sb;            // DE_LOGITS_XB: sequence bias (LAST: every older field keeps its kernel-argument offset)
};

// L2 warm-up workgroup: blockIdx >= n_tiles of the compute grid.  Workgroup n_tiles + t reads tile t of
// the NEXT launch's weight matrix.  Dispatch places block b on XCD b % 8 (observed, not guaranteed --
// a wrong guess only costs speed) and n_tiles % 8 == 0, so tile t lands in the L2 of the XCD whose
// workgroup t will consume it; L2 contents survive the kernel boundary (measured: a GEMV whose
// weights are L2-resident is 0.7-2.0 us shorter).  Runs on CUs the skinny GEMV leaves idle.
__device__ __forceinline__ void l2_warm_tile(const char *base, long tile_bytes, int tile, int nthreads) {
    const u32x4 *src = (const u32x4 *)(base + (long)tile * tile_bytes);
    const long n16 = tile_bytes >> 4;
    for (long i = threadIdx.x; i < n16; i += (long)nthreads * 8) {
        u32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long j = i + (long)u * nthreads;
            v[u] = src[j < n16 ? j : i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("" ::"v"(v[u]));
    }
}

// merged head-output element of a (sequence, head) pair from its NS stream partials (m, l, o): the ONE place the merge
// arithmetic is written -- the attention kernel's own tail and the combine launch both call it, so the launch shapes give
// the same bits
template <int NS>
__device__ __forceinline__ float attn_merge_core(const float (&m)[NS], const float (&l)[NS], const float (&o)[NS]) {
    float M = m[0];
#pragma unroll
    for (int w = 1; w < NS; ++w) M = fmaxf(M, m[w]);
    float acc = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        const float f = __expf(m[w] - M);  // a stream that saw no row has m = -1e30, l = 0, o = 0
        acc = __fmaf_rn(o[w], f, acc);
        L = __fmaf_rn(l[w], f, L);
    }
    return acc / L;
}

// The decode GEMV (round 2): out[b][n] = sum_k a[b][k] W[n][k] for a decode group of any size.
//   * a workgroup owns TN adjacent 16-row weight tiles and NBLK blocks of 16 batch rows; its NW waves split K (SPW
//     k-steps of 32 each -- the split depends on K only, never on the batch or on TN / NBLK, so a row's sum is formed in
//     the same order whatever group it is decoded in and however the launch is shaped);
//   * EVERYTHING the workgroup needs is requested up front -- weights (TN x SPW KiB per wave), the bf16 activation
//     fragments of all its batch blocks straight from L2 in MFMA A-operand order, and the epilogue operands -- so the
//     kernel has ONE memory round trip on its critical path whatever the batch; large batches are covered by more
//     workgroups per tile group (bgroups) and wider tile groups (TN: an activation fragment feeds TN products, which
//     divides the L2 -> CU traffic of the activations), never by a serial loop;
//   * LayerNorm is FOLDED: gamma lives in the weights (W' = W g), so the product runs on the raw bf16 residual and the
//     row statistics enter in the epilogue, out = rstd (a W'^T - mean c1) + c2 -- they arrive as deterministic per-tile
//     partial sums of the f32 residual from whoever wrote it last and are off the critical path;
//   * cross-wave (split-K) sums through LDS in wave order, one barrier; the TN x NBLK (tile, block) units are spread
//     over the waves for the fused epilogue: bias / GELU / residual (+ bf16 copy + partial statistics) / KV append /
//     arg-max (+ suppress bitmaps, timestamp rules).
// LDS carve (dynamic): red [NW][TN*NBLK][64][4] f32 | st [NW][16][2] f32
// repetition rules (DE_LOGITS_XR only: an empty base everywhere else): the bitmap words of the lane's four rows for this tile
template <int EPI>
struct GemvRepWords {};
template <>
struct GemvRepWords<DE_LOGITS_XR> {
    unsigned rseen[4], rban[4];
};
template <>
struct GemvRepWords<DE_LOGITS_XB> : GemvRepWords<DE_LOGITS_XR> {};
// sequence bias (DE_LOGITS_XB only, an empty base everywhere else, for the reason DESIGN.md section 14 gives): the hit words
template <int EPI>
struct GemvSbWords {};
template <>
struct GemvSbWords<DE_LOGITS_XB> {
    unsigned rhit[4];
    int roff[4];   // list index of the word's first hit id (WmSbEpi::woff)
};
template <int EPI, bool LN>
struct GemvUnitOps : GemvRepWords<EPI>, GemvSbWords<EPI> {
    float c1v, c2v;
    float xold[4];
    float off4[4];   // DE_RESID: mean-centring offsets of the lane's four rows
    float offrow;    // LayerNorm modes: offset of row (lane & 15) of the block
    int4 trng[4];
    float2 sv[LN ? 20 : 1];  // statistics parts per lane group: d/16 <= 80 parts
};

// (r0, r1): the accumulator rows (of the lane's four) this wave will finish -- see "ROW SPLIT" in dec_gemv_kernel;
// want_stats: this wave also forms the unit's LayerNorm statistics (one wave per unit)
template <int EPI, bool LN>
__device__ __forceinline__ void gemv_unit_load(const DecGemvDev &p, GemvUnitOps<EPI, LN> &o, int tile, int b0, int lane,
                                               int r0 = 0, int r1 = 4, bool want_stats = true) {
    const int nrow = lane & 15, kq = lane >> 4;
    const int n = tile * 16 + nrow;
    const int nc = n < p.N ? n : p.N - 1;
    const int nb = p.B - b0 < 16 ? p.B - b0 : 16;
    o.c1v = 0.f;
    o.c2v = p.c2 ? p.c2[nc] : 0.f;
    if (LN) o.c1v = p.c1[nc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        o.xold[r] = 0.f;
        o.off4[r] = 0.f;
        o.trng[r] = make_int4(0, 0, 0, 0);
    }
    o.offrow = 0.f;
    if (EPI == DE_RESID) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < r0 || r >= r1) continue;
            const int bl = kq * 4 + r;
            const int bc = b0 + (bl < nb ? bl : nb - 1);
            o.xold[r] = p.out_f32[(long)bc * p.ldo + nc];
            if (p.mean_in) o.off4[r] = p.mean_in[bc];
        }
    }
    if (LN && p.mean_in && want_stats) o.offrow = p.mean_in[b0 + (nrow < nb ? nrow : nb - 1)];
    if (de_is_logits(EPI) && p.ts.rng) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < r0 || r >= r1) continue;
            const int bl = kq * 4 + r;
            o.trng[r] = *(const int4 *)(p.ts.rng + (long)(b0 + (bl < nb ? bl : nb - 1)) * 4);
        }
    }
    if constexpr (de_has_rep(EPI)) {
        // the 16 ids of a tile share ONE bitmap word per row; rows past the group's are clamped like the ranges above
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < r0 || r >= r1) continue;
            const int bl = kq * 4 + r;
            const long wi = (long)(b0 + (bl < nb ? bl : nb - 1)) * p.rep.words + (nc >> 5);
            o.rseen[r] = p.rep.seen[wi];
            o.rban[r] = p.rep.ban[wi];
            if constexpr (EPI == DE_LOGITS_XB) {
                const long si = (long)(b0 + (bl < nb ? bl : nb - 1)) * p.sb.words + (nc >> 5);
                o.rhit[r] = p.sb.hit[si];
                o.roff[r] = p.sb.woff[si];
            }
        }
    }
    if (LN) {
        // all K/16 parts of the block are valid (the embedding kernels zero the ones they do not write), K/16 is a
        // multiple of 4: every lane group reads K/64 of them, a wave-uniform count
        const float *sp = p.stats_in + (long)(b0 >> 4) * p.stats_stride + (kq * 16 + nrow) * 2;
        const int nu = p.K >> 6;
#pragma unroll
        for (int u = 0; u < 20; ++u) {
            o.sv[u] = make_float2(0.f, 0.f);
            if (u < nu && want_stats) o.sv[u] = *(const float2 *)(sp + u * 128);
        }
    }
}

// rstd / -mean rstd of the unit's 16 rows from the partial sums -> wave-private LDS (st), so that every lane can read
// the four rows its accumulator registers hold.  The partial sums were written in a FIXED slab order by the producer
// of the residual, so this sum is deterministic and needs no atomics.
template <int EPI, bool LN>
__device__ __forceinline__ void gemv_unit_stats(const DecGemvDev &p, const GemvUnitOps<EPI, LN> &o, float *st, int lane,
                                                int tile, int b0) {
    if (!LN) return;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < 20; ++u) {
        s1 += o.sv[u].x;
        s2 += o.sv[u].y;
    }
    s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
    s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
    const float mean = s1 / (float)p.K;
    float var = s2 / (float)p.K - mean * mean;
    var = var > 0.f ? var : 0.f;
    const float rstd = rsqrtf(var + 1e-5f);
    if (lane < 16) {
        // the activations are stored as bf16(x - off): the fold needs (mean - off) where it had mean
        *(float2 *)(st + lane * 2) = make_float2(rstd, -(mean - o.offrow) * rstd);
        if (tile == 0 && p.mean_out && b0 + lane < p.B) p.mean_out[b0 + lane] = mean;  // one writer per row
    }
}

// word k of quad lane R's Philox output, for the lane whose index in the quad is k (= its id n & 3): four DPP broadcasts
template <int R>
__device__ __forceinline__ void quad_words(const wm_philox4 &w, int k, unsigned &out) {
    const unsigned w0 = (unsigned)__builtin_amdgcn_mov_dpp((int)w.v[0], R * 0x55, 0xf, 0xf, false);
    const unsigned w1 = (unsigned)__builtin_amdgcn_mov_dpp((int)w.v[1], R * 0x55, 0xf, 0xf, false);
    const unsigned w2 = (unsigned)__builtin_amdgcn_mov_dpp((int)w.v[2], R * 0x55, 0xf, 0xf, false);
    const unsigned w3 = (unsigned)__builtin_amdgcn_mov_dpp((int)w.v[3], R * 0x55, 0xf, 0xf, false);
    const unsigned lo = (k & 1) ? w1 : w0, hi = (k & 1) ? w3 : w2;
    out = (k & 2) ? hi : lo;
}

// the value quad lane R holds, for every lane of the quad
template <int R>
__device__ __forceinline__ float quad_bcast(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), R * 0x55, 0xf, 0xf, false));
}

// ---- the pieces of the logits epilogues (DE_LOGITS*), each stated ONCE.  The 16 lanes that share kq hold the 16 ids of the
// tile for one batch row; their butterflies walk q = 1, 2, 4, 8.  (Which arm calls which, and why not all: DESIGN.md section 4.)
// index of (row b, tile) in the per-tile arrays: tilemax, ts.key_ts, ts.lse, x.txt / x.win / x.all
__device__ __forceinline__ long tile_index(const DecGemvDev &p, int b, int tile) { return (long)b * p.n_tiles + tile; }
// id n is not suppressed: bit n of the row's bitmap word -- the second bitmap at mask_first_pos; zero when no filter is set
__device__ __forceinline__ bool id_allowed(const DecGemvDev &p, int pos, unsigned mword0, unsigned mword1, int n) {
    const unsigned mw = (pos == p.mask_first_pos) ? mword1 : mword0;
    return !((mw >> (n & 31)) & 1u);
}
// id n against a row's timestamp rules (WmTsDev::rng): allowed text [x, y), allowed timestamps [z, w)
__device__ __forceinline__ bool in_text_range(const int4 &rng, int n) { return n >= rng.x && n < rng.y; }
__device__ __forceinline__ bool in_ts_range(const int4 &rng, int n) { return n >= rng.z && n < rng.w; }
// the tile's (max, sum exp) partial of v over the lanes with `in` set (none: (-1e30, 0))
__device__ __forceinline__ float2 tile_lse(bool in, float v) {
    float mx = in ? v : -1e30f;
#pragma unroll
    for (int q = 1; q < 16; q <<= 1) mx = fmaxf(mx, __shfl_xor(mx, q));
    float se = in ? __expf(v - mx) : 0.f;
#pragma unroll
    for (int q = 1; q < 16; q <<= 1) se += __shfl_xor(se, q);
    return make_float2(mx, se);
}
// the 16-lane maximum of two keys, each with a value carried beside it (the extended decode: the winners' RAW logits)
__device__ __forceinline__ void tile_key_max_carry(unsigned long long &kt, float &vt, unsigned long long &ks, float &vs) {
#pragma unroll
    for (int q = 1; q < 16; q <<= 1) {
        const unsigned long long a = __shfl_xor(kt, q), c = __shfl_xor(ks, q);
        const float av = __shfl_xor(vt, q), cv = __shfl_xor(vs, q);
        if (a > kt) { kt = a; vt = av; }
        if (c > ks) { ks = c; vs = cv; }
    }
}
// the tile's timestamp partial: best allowed timestamp and the (max, sum exp) of the allowed timestamps' raw logits (only
// tiles that reach into the timestamp range carry it)
__device__ __forceinline__ void store_ts_partial(const DecGemvDev &p, long ti, unsigned long long ks, float2 lse) {
    p.ts.key_ts[ti] = ks;
    *(float2 *)(p.ts.lse + ti * 2) = lse;
}
// the logits row, when the caller asked for it
__device__ __forceinline__ void store_logit(const DecGemvDev &p, int b, int n, float v) {
    if (p.out_f32) p.out_f32[(long)b * p.ldo + n] = v;
}

// epilogue of one (tile, block) unit by one wave: D col n = lane & 15, rows b = b0 + kq*4 + r
template <int EPI, bool LN>
__device__ __forceinline__ void gemv_unit_epilogue(const DecGemvDev &p, const GemvUnitOps<EPI, LN> &o, const f32x4 acc,
                                                   const float *st, int tile, int b0, int lane, int pos, unsigned mword0,
                                                   unsigned mword1, int r0 = 0, int r1 = 4) {
    const int nrow = lane & 15, kq = lane >> 4;
    const int n0 = tile * 16, n = n0 + nrow;
    const bool nvalid = n < p.N;
    const int nb = p.B - b0 < 16 ? p.B - b0 : 16;
    unsigned draw[4] = {0u, 0u, 0u, 0u};   // DE_LOGITS_X under sampling: the 32-bit draw of (row kq * 4 + r, id n)
    float inv_t[4] = {0.f, 0.f, 0.f, 0.f};   // ... and the row's 1 / T: the call's, or the row's own (WmXPar::rows_on; 0: an arg-max row)
    if (de_is_x(EPI)) {
        const WmXPar xp = *p.x.par;
        const int gi = pos + 1 - xp.n_prompt;
        if (xp.sample && gi >= 0) {   // wave-uniform (every lane active); with a row table: some row of the call samples
            // ONE Philox call serves the four ids of a quad (lanes 4q .. 4q + 3 = ids 4 (n >> 2) .. + 3) for one row: lane j
            // of the quad runs the call of row kq * 4 + j, and DPP broadcasts hand every lane its word (n & 3) of each row's call
            const int j = nrow & 3;
            wm_philox4 c;
            const int row = b0 + kq * 4 + j;   // (rows past the group's: their draws are never used)
            c.v[0] = (unsigned)n >> 2; c.v[1] = (unsigned)gi; c.v[2] = xp.ids_on ? p.x.ids[row] : (unsigned)(xp.chunk0 + row);
            c.v[3] = xp.n_cand > 1 ? p.x.ids[WM_XIDS_CAND + row] : 0u;   // the candidate word (best-of-N; 0 in every other call)
            unsigned k0 = xp.key0, k1 = xp.key1;
            float it = xp.inv_T;
            if (xp.rows_on) {   // wave-uniform: the call of row kq * 4 + j takes that row's key (the table is padded like ids)
                const WmXRow rw = wm_x_rows(p.x.ids)[row];
                k0 = rw.key0; k1 = rw.key1; it = rw.inv_T;
            }
            const wm_philox4 w = wm_philox4x32_10(c, k0, k1);
            quad_words<0>(w, j, draw[0]);
            quad_words<1>(w, j, draw[1]);
            quad_words<2>(w, j, draw[2]);
            quad_words<3>(w, j, draw[3]);
            // lane j holds 1 / T of row kq * 4 + j: one more broadcast per row (without a table: four copies of the call's)
            inv_t[0] = quad_bcast<0>(it);
            inv_t[1] = quad_bcast<1>(it);
            inv_t[2] = quad_bcast<2>(it);
            inv_t[3] = quad_bcast<3>(it);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r < r0 || r >= r1) continue;  // wave-uniform: this wave's share of the unit's rows
        const int bl = kq * 4 + r;
        const int b = b0 + bl;
        const bool bvalid = bl < nb;
        float v;
        if (LN) {
            const float2 ms = *(const float2 *)(st + bl * 2);
            v = __fmaf_rn(ms.x, acc[r], __fmaf_rn(ms.y, o.c1v, o.c2v));  // rstd (acc - mean c1) + c2
        } else {
            v = acc[r] + o.c2v;
        }
        bool rbanned = false;
        const float vraw = v;   // DE_LOGITS_XB: no_speech_prob is read from the raw logits
        if constexpr (de_has_rep(EPI)) {
            // repetition rules first: the penalised value REPLACES the logit for everything below (keys, scores, partials,
            // the winners' raw logits, the stored row); a banned id is treated like a suppressed one.  The bitmaps hold ids
            // < eot only (wm_repeat_state) and are empty at a prompt position.
            const WmRepPar rp = *p.rep.par;
            const unsigned bit = 1u << (n & 31);
            if (o.rseen[r] & bit) v = v > 0.f ? __fmul_rn(v, rp.inv_p) : __fmul_rn(v, rp.p);
            rbanned = (o.rban[r] & bit) != 0u;
            if constexpr (EPI == DE_LOGITS_XB) {
                // sequence bias behind the penalty: v + total(n), ONE f32 add for every id (total = +0.0f without a matching
                // entry); only a set hit bit pays for the lookup, ONE load: the list is sorted by id, so the id's place in it is
                // the word's offset + the hit bits below the id.  A banned id has total -inf and its ban bit set.
                float tot = 0.f;
                if (o.rhit[r] & bit) {
                    int at = o.roff[r] + __popc(o.rhit[r] & (bit - 1u));
                    at = at < 0 ? 0 : (at < WM_MAX_BIAS_ENTRIES ? at : WM_MAX_BIAS_ENTRIES - 1);
                    tot = p.sb.ltot[(long)(b0 + (bl < nb ? bl : nb - 1)) * WM_MAX_BIAS_ENTRIES + at];
                }
                v = __fadd_rn(v, tot);
            }
        }
        if (de_is_x(EPI)) {
            // extended decode: the DE_LOGITS keys (timestamp rules or the plain [arg_first, arg_last] range), over
            // Gumbel-perturbed scores when sampling, with the winners' RAW logits beside them (their log-probs; score - g
            // would lose bits), plus the (max, sum exp) partial of the allowed text ids and, at the <|startoftranscript|>
            // position only, the unfiltered one over the whole vocabulary (no_speech_prob).  Wave-uniform branches.
            const WmXPar xp = *p.x.par;
            const bool ok = bvalid && nvalid && id_allowed(p, pos, mword0, mword1, n) && !(de_has_rep(EPI) && rbanned);
            const bool ts_on = p.ts.rng != nullptr;
            const bool in_text = ts_on ? (ok && in_text_range(o.trng[r], n)) : (ok && n >= p.arg_first && n <= p.arg_last);
            const bool in_ts = ts_on && ok && in_ts_range(o.trng[r], n);
            const int gi = pos + 1 - xp.n_prompt;
            float sc = v;
            // (a row of a table whose 1 / T is zero is an arg-max row: its score is the logit, bit for bit the temperature-0 call's)
            if (xp.sample && gi >= 0 && !(xp.rows_on && __float_as_uint(inv_t[r]) == 0u))
                sc = __fmaf_rn(v, inv_t[r], wm_gumbel_from_bits(draw[r]));
            unsigned long long kt = in_text ? argmax_key(sc, n) : 0ull, ks = in_ts ? argmax_key(sc, n) : 0ull;
            float vt = v, vs = v;
            tile_key_max_carry(kt, vt, ks, vs);
            const float2 lt = tile_lse(in_text, v);
            const long ti = tile_index(p, b, tile);
            if (bvalid && nrow == 0) {
                p.tilemax[ti] = kt;
                *(float2 *)(p.x.txt + ti * 2) = lt;
                *(float2 *)(p.x.win + ti * 2) = make_float2(vt, vs);
            }
            if (ts_on && n0 + 16 > p.ts.ts_begin) {  // wave-uniform: the DE_LOGITS timestamp partial (raw logits)
                const float2 ls = tile_lse(in_ts, v);
                if (bvalid && nrow == 0) store_ts_partial(p, ti, ks, ls);
            }
            if (pos == xp.sot_pos) {  // wave-uniform: openai-whisper reads no_speech_prob before any filter
                const float vn = EPI == DE_LOGITS_XB ? vraw : v;   // (the history is empty here: the penalty has not touched it)
                const float2 la = tile_lse(bvalid && nvalid, vn);
                if (bvalid && nrow == 0) *(float2 *)(p.x.all + ti * 2) = la;
                if (bvalid && n == xp.ns_tok) p.x.ns_v[b] = vn;
            }
            if (bvalid && nvalid) store_logit(p, b, n, v);
            continue;
        }
        if (EPI == DE_LOGITS && p.ts.rng) {
            // timestamp rules: best allowed text token, best allowed timestamp, and the (max, sum exp) partial of the
            // allowed timestamps of this tile (only tiles that reach into the timestamp range carry the last two)
            const bool ok = bvalid && nvalid && id_allowed(p, pos, mword0, mword1, n);
            const bool in_text = ok && n >= o.trng[r].x && n < o.trng[r].y;
            const bool in_ts = ok && n >= o.trng[r].z && n < o.trng[r].w;
            unsigned long long kt = in_text ? argmax_key(v, n) : 0ull, ks = in_ts ? argmax_key(v, n) : 0ull;
#pragma unroll
            for (int q = 1; q < 16; q <<= 1) {
                const unsigned long long a = __shfl_xor(kt, q), c = __shfl_xor(ks, q);
                kt = a > kt ? a : kt;
                ks = c > ks ? c : ks;
            }
            if (bvalid && nrow == 0) p.tilemax[tile_index(p, b, tile)] = kt;
            if (n0 + 16 > p.ts.ts_begin) {  // wave-uniform
                const float2 ls = tile_lse(in_ts, v);
                if (bvalid && nrow == 0) {
                    p.ts.key_ts[(long)b * p.n_tiles + tile] = ks;
                    *(float2 *)(p.ts.lse + ((long)b * p.n_tiles + tile) * 2) = ls;
                }
            }
            if (bvalid && nvalid) store_logit(p, b, n, v);
            continue;
        }
        if (EPI == DE_LOGITS) {
            // arg-max over [arg_first, arg_last], first maximal index wins (Whisper.swift:38)
            unsigned long long key = 0ull;
            if (bvalid && nvalid && n >= p.arg_first && n <= p.arg_last && id_allowed(p, pos, mword0, mword1, n)) key = argmax_key(v, n);
#pragma unroll
            for (int q = 1; q < 16; q <<= 1) {
                const unsigned long long ok = __shfl_xor(key, q);
                key = ok > key ? ok : key;
            }
            if (bvalid && nrow == 0) p.tilemax[tile_index(p, b, tile)] = key;
            if (bvalid && nvalid) store_logit(p, b, n, v);
            continue;
        }
        if (EPI == DE_RESID) {
            // residual update (f32 + the bf16 copy the next GEMV multiplies) + this tile's partial LayerNorm
            // statistics of the updated rows
            float xn = 0.f;
            if (bvalid && nvalid) {
                xn = o.xold[r] + v;
                p.out_f32[(long)b * p.ldo + n] = xn;
                if (p.out_bf16) p.out_bf16[wm_tiled_offset((size_t)b, (size_t)n, (size_t)p.ldo)] = f2bf(xn - o.off4[r]);
            }
            float s1 = xn, s2 = xn * xn;
#pragma unroll
            for (int q = 1; q < 16; q <<= 1) {
                s1 += __shfl_xor(s1, q);
                s2 += __shfl_xor(s2, q);
            }
            if (p.stats_out && nrow == 0)
                *(float2 *)(p.stats_out + (long)(b0 >> 4) * p.stats_stride + ((long)tile * 16 + bl) * 2) = make_float2(s1, s2);
            continue;
        }
        if (!bvalid || !nvalid) continue;
        if (EPI == DE_QKV) {
            const int d = p.N / 3;
            if (n < d) {
                p.out_f32[(long)b * d + n] = v;
            } else {
                const int hn = (n < 2 * d) ? n - d : n - 2 * d;
                bf16_t *c = (n < 2 * d) ? p.kcache : p.vcache;
                c[((long)(b * p.n_head + (hn >> 6)) * p.n_ctx + pos) * 64 + (hn & 63)] = f2bf(v);
            }
        } else if (EPI == DE_Q) {
            p.out_f32[(long)b * p.ldo + n] = v;
        } else if (EPI == DE_GELU) {
            p.out_bf16[wm_tiled_offset((size_t)b, (size_t)n, (size_t)p.ldo)] = f2bf(gelu_erf(v));
        } else if (EPI == DE_QKV_P) {
            // a panel step: row b = (window b / w, position pos + b % w) -- the query stays row b's, k / v are appended to the
            // WINDOW's cache entry at the row's own position (< n_ctx by the host's cut of the pass; checked all the same)
            const int d = p.N / 3;
            if (n < d) {
                p.out_f32[(long)b * d + n] = v;
            } else {
                const int hn = (n < 2 * d) ? n - d : n - 2 * d;
                bf16_t *c = (n < 2 * d) ? p.kcache : p.vcache;
                const int cw = b / p.panel, ps = pos + (b - cw * p.panel);
                if (ps < p.n_ctx) c[((long)(cw * p.n_head + (hn >> 6)) * p.n_ctx + ps) * 64 + (hn & 63)] = f2bf(v);
            }
        }
    }
}

// PPW (parts per wave): 1 = every wave owns one K part, all loads up front (the latency shape).  2 = a wave walks TWO
// parts one after the other (part w, then part w + NW) in the same registers: half the waves per workgroup for the same
// K split, so the 16-part K = 4d product runs as an 8-wave workgroup of <= 128 VGPRs that sits TWO per CU -- at more
// than one batch block its (tile, block) grid then fits one residency round of the chip instead of two (one extra L2
// round trip inside the workgroup, a whole kernel time saved).  The parts, their MFMA chains and the order they are
// added in are the same: bit-identical results.
// KERNEL ARGUMENTS (round 5).  The compiler fetches the fields of a by-value struct lazily, one s_load per first use: the
// round-4 kernel walked FOUR dependent scalar round trips (bgroups -> n_tg -> pf fields -> W, a, K) before its first weight
// load was even issued, and a scalar load of a fresh dispatch misses the scalar cache (invalidated at the kernel boundary).
// Now everything on the path to the first weight load is a leading SCALAR parameter: one s_load burst at most, and with
// -mllvm -amdgpu-kernarg-preload-count=16 (build.py, this file only: 16 = the upper bound; the GEMV's 14 leading dwords
// of hot scalars are what fits and is preloaded) the dispatcher places them in SGPRs before the first instruction (a by-value struct is never preloaded).  The cold fields stay in the struct; they are
// requested in one burst right after the weight / activation loads (GEMV_PIN below).
#define GEMV_PIN(x) asm volatile("" ::"s"(x))
template <int SPW, int TN, int NBLK, int EPI, bool LN, int PPW = 1, int RSP = 1>
__global__ __launch_bounds__((LN || SPW == 12 || TN * NBLK > 1 || PPW > 1) ? 512 : 1024) void dec_gemv_kernel(
    const bf16_t *__restrict__ hotW, const bf16_t *__restrict__ hotA, const int *__restrict__ hot_pos_ptr,
    const float *__restrict__ hot_c2, int hotK, int hot_n_tiles, int hotB, int hot_bgroups, int hot_n_tg, int hot_n_tg_pad,
    float *hot_out_f32, DecGemvDev pc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DecGemvDev p = pc;  // (scalarised by the compiler: a field is a kernarg load at its first use)
    p.W = hotW; p.a = hotA; p.pos_ptr = hot_pos_ptr; p.c2 = hot_c2; p.K = hotK; p.n_tiles = hot_n_tiles; p.B = hotB;
    p.bgroups = hot_bgroups; p.n_tg = hot_n_tg; p.n_tg_pad = hot_n_tg_pad; p.out_f32 = hot_out_f32;
    constexpr int NU = TN * NBLK;
    const int NP = (p.K >> 5) / SPW;  // K parts (blockDim.x lives in the hidden kernel arguments: one more scalar round trip)
    const int NW = NP / PPW;
    // Workgroup id -> (tile group, batch group): ids 8q .. 8q+7 are tile groups 8(q / G) .. +7 of batch group q % G, so
    // the workgroups of a tile group are dispatched back to back AND on the same XCD (id % 8): the later ones read the
    // weights from the L2 the first one filled -- one HBM stream per tile.  (G == 1: id == tile group.)
    const int G = p.bgroups;
    const int wg = blockIdx.x;
    const int q = wg >> 3;
    const int tg = G == 1 ? wg : (q / G) * 8 + (wg & 7);
    const int grp = G == 1 ? 0 : q % G;
    if (wg >= p.n_tg_pad * G || tg >= p.n_tg) {  // workgroup-uniform: warm-up workgroups and padding
        int t = wg - p.n_tg_pad * G;   // (warm-up workgroups exist only when n_tg_pad * G % 8 == 0, wm_dec_gemv: t & 7 == wg & 7, this workgroup's XCD)
        if (p.pf_head_major && t >= 0) {
            // the next launch is the fused query + cross-attention kernel (dec_xattn_fq_kernel): XCD x runs the pairs
            // [x per, (x + 1) per) of the head-major pair list (per = pf_head_major), i.e. a few whole or half heads --
            // warm-up workgroup 8 m + x (on XCD x) pulls tile m % 4 of the (m / 4)-th head that XCD x hosts
            const int per = p.pf_head_major, x = t & 7, m = t >> 3;
            const int hh = (x * per) / p.B + (m >> 2);
            const int end = (x + 1) * per < (p.pf_tiles >> 2) * p.B ? (x + 1) * per : (p.pf_tiles >> 2) * p.B;
            t = hh * p.B < end ? hh * 4 + (m & 3) : -1;
        }
        if (t >= 0 && t < p.pf_tiles) l2_warm_tile(p.pf_ptr, p.pf_tile_bytes, t, NW * 64);
        return;
    }
    float *red = (float *)smem;
    float *st = red + NP * NU * 256 + (threadIdx.x >> 6) * 32;  // wave-private
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrow = lane & 15;
    const int tile0 = tg * TN;
    const int bb = grp * NBLK * 16;  // first batch row of this workgroup (< B by construction of the grid)

    // ---- 1. every load of the workgroup in flight: weights (fragment-tiled: k-step s of n-tile t is the contiguous
    // KiB at ((t * K/32 + s) * 64 + lane) * 8 -- one perfectly coalesced dwordx4 per lane per step) ...
    u32x4 wf[TN][SPW];
    auto load_wf = [&](int part) {
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const int tc = tile0 + t < p.n_tiles ? tile0 + t : p.n_tiles - 1;  // clamped: unconditional loads
            const bf16_t *wp = p.W + (((long)tc * (p.K >> 5) + (long)part * SPW) * 64 + lane) * 8;
#pragma unroll
            // plain (cacheable) loads, not non-temporal ones: a decode group reads a weight matrix once per position, but the
            // groups in flight walk the same layers a few layers apart, and the second and third reader find the matrix in the
            // 256 MB Infinity Cache (measured, 3 groups of 56: 2000 -> 2055 audio-s/s; one group alone: no difference)
#ifdef WM_GEMV_W_NONTEMPORAL
            for (int u = 0; u < SPW; ++u) wf[t][u] = __builtin_nontemporal_load((const u32x4 *)(wp + u * 512));
#else
            for (int u = 0; u < SPW; ++u) wf[t][u] = *(const u32x4 *)(wp + u * 512);
#endif
        }
    };
    load_wf(wave);
    // ... the activation fragments of its batch blocks: the activations are stored fragment-tiled exactly like the
    // weights (block of 16 rows x k-step = one contiguous KiB in MFMA A-operand order, written that way by their
    // producers), so this is ONE perfectly coalesced dwordx4 per lane per step too -- a row-major [B][K] buffer costs
    // 16 half-used cache lines per wave-load and twice the L2 -> CU traffic.  Rows past B inside the last block hold
    // stale data: an MFMA output row depends on its own A row only, and those rows are never stored ...
    u32x4 af[NBLK][SPW];
    auto load_af = [&](int part) {
#pragma unroll
        for (int j = 0; j < NBLK; ++j) {
            const int blk = (bb >> 4) + j;
            const int blkc = blk * 16 < p.B ? blk : (bb >> 4);  // a missing second block re-reads the first (never used)
            const bf16_t *ap = p.a + (((long)blkc * (p.K >> 5) + (long)part * SPW) * 64 + lane) * 8;
#pragma unroll
            for (int u = 0; u < SPW; ++u) af[j][u] = *(const u32x4 *)(ap + u * 512);
        }
    };
    load_af(wave);
    // ... the cold kernel arguments, ONE scalar burst behind the loads above ...
    GEMV_PIN(p.N); GEMV_PIN(p.ldo);
    if (LN) { GEMV_PIN(p.c1); GEMV_PIN(p.stats_in); GEMV_PIN(p.stats_stride); GEMV_PIN(p.mean_in); GEMV_PIN(p.mean_out); }
    if (EPI == DE_RESID) { GEMV_PIN(p.out_bf16); GEMV_PIN(p.stats_out); GEMV_PIN(p.stats_stride); GEMV_PIN(p.mean_in); }
    if (EPI == DE_QKV || EPI == DE_QKV_P) { GEMV_PIN(p.kcache); GEMV_PIN(p.vcache); GEMV_PIN(p.n_ctx); GEMV_PIN(p.n_head); }
    if (EPI == DE_QKV_P) GEMV_PIN(p.panel);
    if (EPI == DE_GELU) GEMV_PIN(p.out_bf16);
    if (de_has_rep(EPI)) { GEMV_PIN(p.rep.par); GEMV_PIN(p.rep.seen); GEMV_PIN(p.rep.ban); GEMV_PIN(p.rep.words); }
    if (EPI == DE_LOGITS_XB) { GEMV_PIN(p.sb.hit); GEMV_PIN(p.sb.woff); GEMV_PIN(p.sb.ltot); GEMV_PIN(p.sb.words); }
    if (de_is_logits(EPI)) {
        GEMV_PIN(p.tilemax); GEMV_PIN(p.arg_first); GEMV_PIN(p.arg_last); GEMV_PIN(p.mask); GEMV_PIN(p.mask_words);
        GEMV_PIN(p.mask_first_pos); GEMV_PIN(p.ts.rng); GEMV_PIN(p.ts.key_ts); GEMV_PIN(p.ts.lse); GEMV_PIN(p.ts.ts_begin);
    }
    // ... and the epilogue operands of the (tile, block) unit this wave will finish: unit u = j * TN + t -> wave u % NW
    // ROW SPLIT (round 5, template RSP = 4).  The epilogue of a (tile, block) unit used to be ONE wave's work while the
    // workgroup's other waves had already finished: ~200 dependent instructions (shuffles for the statistics, scattered
    // bf16 / f32 stores) at one wave's issue rate -- the out-projection (residual epilogue) took 0.9 us longer than the
    // query projection on the same matrix.  In the RESIDUAL kernels, when the workgroup has at least four waves per unit
    // and more than one sequence, a unit's four accumulator rows per lane (batch rows kq * 4 + r) are finished by FOUR
    // waves, one r each: wave 4 u + r takes row r of unit u.  Same instructions per element, same order of the split-K sum:
    // same bits.  (A compile-time choice per launch: as a run-time switch in every kernel it cost the LayerNorm GEMVs,
    // whose epilogue is a single fma per row, 0.3 us each -- profiles/r05_latency_probe.txt.)
    int pos = 0;
    unsigned mword0 = 0u, mword1 = 0u;
    GemvUnitOps<EPI, LN> ops;
    constexpr int RS = RSP;                     // waves per unit in the epilogue
    static_assert(RSP == 1 || RSP == 4, "row split: 1 or 4 waves per unit");
    constexpr int rs_shift = RS == 4 ? 2 : 0;
    const int ntask = NU << rs_shift;
    const bool has_unit = wave < ntask;         // wave-uniform: this wave finishes (part of) a unit
    const int my_u = wave >> rs_shift;
    const int my_r0 = RS == 4 ? (wave & 3) : 0, my_r1 = RS == 4 ? my_r0 + 1 : 4;
    const bool my_stats = my_r0 == 0;           // the wave that forms the unit's LayerNorm statistics
    int utile = tile0, ub0 = bb;
    if (has_unit) {
        utile = tile0 + my_u % TN;
        ub0 = bb + (my_u / TN) * 16;
        if (utile >= p.n_tiles) utile = p.n_tiles - 1;
        if (ub0 >= p.B) ub0 = bb;
        gemv_unit_load<EPI, LN>(p, ops, utile, ub0, lane, my_r0, my_r1, my_stats);
    }
    if (p.pos_ptr) pos = *p.pos_ptr;
    if (de_is_logits(EPI) && p.mask && has_unit) {
        const int n = utile * 16 + nrow;
        const int nc = n < p.N ? n : p.N - 1;
        mword0 = p.mask[nc >> 5];
        mword1 = p.mask[p.mask_words + (nc >> 5)];
    }

    // ---- 2. products of this wave's K part(s): an activation fragment feeds the TN tiles
    // ---- 3. cross-wave (split-K) reduction through LDS, one slot per part; statistics of this wave's unit meanwhile
    f32x4 acc[NBLK][TN];
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int part = wave + pp * NW;
        if (pp > 0) {  // second part: same registers, requested once the first part's products have read them
            load_wf(part);
            load_af(part);
        }
#pragma unroll
        for (int j = 0; j < NBLK; ++j)
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < SPW; ++u)
                    a4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[j][u]),
                                                                 __builtin_bit_cast(bf16x8, wf[t][u]), a4, 0, 0, 0);
                acc[j][t] = a4;
            }
        if (PPW > 1 || NU > 1 || wave != 0 || RS == 4) {  // (wave 0 finishing its own part alone needs no copy of it)
#pragma unroll
            for (int j = 0; j < NBLK; ++j)
#pragma unroll
                for (int t = 0; t < TN; ++t) *(f32x4 *)(red + ((part * NU + j * TN + t) * 64 + lane) * 4) = acc[j][t];
        }
    }
    // the statistics slot of a unit: slot u when its rows are split over four waves (written by wave 4 u before the
    // barrier, read by all four after it), else the finishing wave's own slot
    float *stbase = red + NP * NU * 256;
    if (has_unit && my_stats) gemv_unit_stats<EPI, LN>(p, ops, stbase + (RS == 4 ? my_u : wave) * 32, lane, utile, ub0);
    __syncthreads();
    // ---- 4. fused epilogues: task t = (unit, row share) on wave t % NW (the first task's operands are already here)
    for (int tk = wave; tk < ntask; tk += NW) {  // wave-uniform; RS == 4: at most one trip
        const int u = tk >> rs_shift;
        const int t = u % TN, j = u / TN;
        const int tile = tile0 + t, b0 = bb + j * 16;
        if (tile >= p.n_tiles || b0 >= p.B) continue;
        st = stbase + (RS == 4 ? u : wave) * 32;
        if (tk != wave) {  // more units than waves (small models; RS == 1): operands fetched late
            gemv_unit_load<EPI, LN>(p, ops, tile, b0, lane);
            gemv_unit_stats<EPI, LN>(p, ops, st, lane, tile, b0);
            if (de_is_logits(EPI) && p.mask) {
                const int n = tile * 16 + nrow;
                const int nc = n < p.N ? n : p.N - 1;
                mword0 = p.mask[nc >> 5];
                mword1 = p.mask[p.mask_words + (nc >> 5)];
            }
        }
        f32x4 sum;
        if (RS == 4) {
            // this wave finishes ONE accumulator row of the unit: it reads that component only (eight waves reading whole
            // f32x4 partials were 4 x the LDS traffic of the two-wave epilogue and cost the LayerNorm GEMVs 0.3 - 0.5 us)
            const float *rp = red + (u * 64 + lane) * 4 + my_r0;
            float s1 = rp[0];
            for (int w = 1; w < NP; ++w) s1 += rp[w * NU * 256];
            sum = f32x4{s1, s1, s1, s1};  // (the epilogue looks at component my_r0 only)
        } else {
            sum = (NU == 1 && PPW == 1) ? acc[0][0] : *(const f32x4 *)(red + ((0 * NU + u) * 64 + lane) * 4);
            for (int w = 1; w < NP; ++w) sum += *(const f32x4 *)(red + ((w * NU + u) * 64 + lane) * 4);
        }
        gemv_unit_epilogue<EPI, LN>(p, ops, sum, st, tile, b0, lane, pos, mword0, mword1, my_r0, my_r1);
    }
}

// LayerNorm folding (wm_finalize): W'[n][k] = bf16(W[n][k] g[k]) in the same WL_TILED order, c1[n] = sum_k W'[n][k],
// c2[n] = bias[n] + sum_k beta[k] W[n][k].  One workgroup per weight row; fixed summation order.
__global__ __launch_bounds__(256) void ln_fold_kernel(const bf16_t *__restrict__ W, const float *__restrict__ g,
                                                      const float *__restrict__ beta, const float *__restrict__ bias,
                                                      int N, int K, bf16_t *__restrict__ Wf, float *__restrict__ c1,
                                                      float *__restrict__ c2) {
    __shared__ float r1[4], r2[4];
    const int n = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const size_t o = wm_tiled_offset((size_t)n, (size_t)k, (size_t)K);
        const float w = bf2f(W[o]);
        const bf16_t wf = f2bf(w * g[k]);
        Wf[o] = wf;
        s1 += bf2f(wf);
        s2 += beta[k] * w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if ((threadIdx.x & 63) == 0) {
        r1[threadIdx.x >> 6] = s1;
        r2[threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c1[n] = (r1[0] + r1[1]) + (r1[2] + r1[3]);
        c2[n] = (n < N && bias ? bias[n] : 0.f) + ((r2[0] + r2[1]) + (r2[2] + r2[3]));
    }
}

// ------------------------------------------------------------------ token embedding ------
// x[b] = token_embedding[seq[pos][b]] + positional_embedding[pos]  (+ LayerNorm partial statistics)
// The embedding of a call's FIRST position, one 4-wave workgroup per row.  Every later position is embedded by the launch that
// closes the one before it (embed_row of dec_close.h: ONE wave per row, 64-lane stride).  The two are not one function: the
// four-wave sums here and the one-wave sums there differ in the last place, so merging them would change results.
// off (nullable, [B]): a ragged decode group -- row b's prompt starts at position off[b] of the group, so its positional
// row is pos - off[b] (0 while the row has not started)
// (the four-wave arithmetic as a device function: dec_embed_kernel and the panel embedding's position 0 call it)
__device__ __forceinline__ void embed_first_row(long tok, int prow, int b, const bf16_t *__restrict__ emb,
                                                const float *__restrict__ pemb, int d, float *__restrict__ x,
                                                bf16_t *__restrict__ xb, float *__restrict__ stats_out,
                                                float *__restrict__ mean_buf) {
    __shared__ float r1[4], r2[4];
    float s1 = 0.f, s2 = 0.f;
    for (int j = threadIdx.x; j < d; j += 256) {
        const float v = bf2f(emb[wm_tiled_offset((size_t)tok, (size_t)j, (size_t)d)]) + pemb[(long)prow * d + j];
        x[(long)b * d + j] = v;
        s1 += v;
        s2 += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if ((threadIdx.x & 63) == 0) {
        r1[threadIdx.x >> 6] = s1;
        r2[threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    {   // bf16 copy, mean-centred (see DecGemvDev::mean_in); the row mean is what the first LayerNorm will compute
        const float mean = ((r1[0] + r1[1]) + (r1[2] + r1[3])) / (float)d;
        for (int j = threadIdx.x; j < d; j += 256)
            xb[wm_tiled_offset((size_t)b, (size_t)j, (size_t)d)] = f2bf(x[(long)b * d + j] - mean);
        if (threadIdx.x == 0 && mean_buf) mean_buf[b] = mean;
    }
    // the whole row is ONE part (index 0); the consumers always sum d/16 parts, so the others are zeroed
    if (stats_out) {
        float *blk = stats_out + (long)(b >> 4) * (2 * d) + (b & 15) * 2;  // block of 16 rows: [d/16 parts][16][2]
        for (int pt = 1 + threadIdx.x; pt < d / 16; pt += 256) *(float2 *)(blk + pt * 32) = make_float2(0.f, 0.f);
        if (threadIdx.x == 0)
            *(float2 *)blk = make_float2((r1[0] + r1[1]) + (r1[2] + r1[3]), (r2[0] + r2[1]) + (r2[2] + r2[3]));
    }
}
__global__ __launch_bounds__(256) void dec_embed_kernel(const int *__restrict__ seq, const int *__restrict__ pos_ptr,
                                                        int B, const bf16_t *__restrict__ emb,
                                                        const float *__restrict__ pemb, int d,
                                                        float *__restrict__ x, bf16_t *__restrict__ xb,
                                                        float *__restrict__ stats_out, float *__restrict__ mean_buf,
                                                        const int *__restrict__ off) {
    const int b = blockIdx.x;
    const int pos = *pos_ptr;
    const long tok = seq[pos * B + b];
    const int prow = off ? max(pos - off[b], 0) : pos;
    embed_first_row(tok, prow, b, emb, pemb, d, x, xb, stats_out, mean_buf);
}

// The embedding of a teacher-forced PANEL (wm_set_teacher_panel): one workgroup per row r = c * w + s = (window c, position
// *pos_ptr + pos_add + s).  A row at position 0 is the call's first embedding (the four-wave sums above), every later position
// the embedding a closing launch would have written (embed_row of dec_close.h, ONE wave): per row the bits of the step path.
__global__ __launch_bounds__(256) void dec_embed_panel_kernel(const int *__restrict__ seq, int seq_stride,
                                                              const int *__restrict__ pos_ptr, int pos_add, int w,
                                                              const bf16_t *__restrict__ emb, const float *__restrict__ pemb,
                                                              int d, int n_ctx, float *__restrict__ x, bf16_t *__restrict__ xb,
                                                              float *__restrict__ stats_out, float *__restrict__ mean_buf) {
    const int r = blockIdx.x, c = r / w;
    const int pos = *pos_ptr + pos_add + (r - c * w);
    if (pos >= n_ctx) return;   // (workgroup-uniform; never taken in a pass cut by the host)
    const long tok = seq[(long)pos * seq_stride + c];
    if (pos == 0) {             // workgroup-uniform
        embed_first_row(tok, 0, r, emb, pemb, d, x, xb, stats_out, mean_buf);
    } else if (threadIdx.x < 64) {
        embed_row(tok, pos, r, (int)threadIdx.x, emb, pemb, d, x, xb, stats_out, mean_buf);
    }
}
// ... of a RAGGED group (wm_set_prompt_panel): window c's prompt starts at group position off[c], so the row's positional row
// is max(pos - off[c], 0) -- what dec_embed_kernel writes at group position 0 and the closing launch at every later one.
__global__ __launch_bounds__(256) void dec_embed_panel_off_kernel(const int *__restrict__ seq, int seq_stride,
                                                                  const int *__restrict__ pos_ptr, int pos_add, int w,
                                                                  const bf16_t *__restrict__ emb, const float *__restrict__ pemb,
                                                                  int d, int n_ctx, float *__restrict__ x, bf16_t *__restrict__ xb,
                                                                  float *__restrict__ stats_out, float *__restrict__ mean_buf,
                                                                  const int *__restrict__ off) {
    const int r = blockIdx.x, c = r / w;
    const int pos = *pos_ptr + pos_add + (r - c * w);
    if (pos >= n_ctx) return;   // (workgroup-uniform; never taken in a pass cut by the host)
    const long tok = seq[(long)pos * seq_stride + c];
    const int prow = max(pos - off[c], 0);
    if (pos == 0) {             // workgroup-uniform
        embed_first_row(tok, prow, r, emb, pemb, d, x, xb, stats_out, mean_buf);
    } else if (threadIdx.x < 64) {
        embed_row(tok, prow, r, (int)threadIdx.x, emb, pemb, d, x, xb, stats_out, mean_buf);
    }
}
__global__ void dec_pos_add_kernel(int *pos_ptr, int add) { *pos_ptr += add; }

// ------------------------------------------------------------------ single-query attention
// One kernel serves the decoder's two attentions.  The rows of a (sequence, head) pair are dealt to NS canonical
// STREAMS (NS = 8 for the cross-attention over the 1500 encoder frames, 4 for the causal self-attention over <= 448
// cached rows): row i belongs to stream (i / 8) % NS, 8 lanes share a 128-byte K/V row (16 B each), a wave is one
// stream and walks its rows in blocks of U loads (K and V of a block requested together), keeping its own running
// (max, sum, o[64]) -- no workgroup barrier inside the row loop -- and the NS partial results are merged ONCE, in
// stream order.  fp32 softmax, bf16 head output.
// Which workgroup runs which stream is a launch-shape choice that cannot change a single bit of the result: nsplit
// (1, 2, 4 or 8) workgroups of NS / nsplit waves share a pair when there are too few pairs to fill the chip (they
// leave (m, l, o[64]) per stream in `part` and dec_attn_combine_kernel performs the same merge), one workgroup of NS
// waves takes the whole pair otherwise and writes the head output itself.  Tokens therefore do not depend on the size
// of the decode group (bit-level batch invariance; the round-1 kernels switched arithmetic with the batch).
// NT: non-temporal loads (a cross-attention cache row is read once per step).
constexpr int ATT_MAXK = WM_ATT_MAXK;   // dec_launch.h: the plans check it
#ifndef WM_XATTN_NT
#define WM_XATTN_NT true  // cross-attention K/V rows: non-temporal loads (A/B builds: -DWM_XATTN_NT=false)
#endif

// merged head-output element e of a pair from NS stream partials held in arrays (LDS / HBM): see attn_merge_core
template <int NS>
__device__ __forceinline__ float attn_merge(const float *m, const float *l, const float *o, int ostride, int e) {
    float mm[NS], ll[NS], oo[NS];
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        mm[w] = m[w];
        ll[w] = l[w];
        oo[w] = o[w * ostride + e];
    }
    return attn_merge_core<NS>(mm, ll, oo);
}

// ---- the per-stream arithmetic of the three attention kernels (dec_rows_attn_kernel, dec_xrows_attn_kernel,
// dec_xattn_fq_kernel), written ONCE so that every launch shape gives the same bits.  Each kernel keeps its own prologue,
// loop driver, query load and tail (the stores of the reduced stream and the merge).  Lane geometry: row i of a pair
// belongs to stream (i / 8) % NS; lane 8 rg + e8 of the stream's wave holds 16 bytes (columns e8 * 8 .. e8 * 8 + 7) of the
// block's rows with i % 8 == rg.
// Machine code: a kernel calls attn_load_block / attn_block from its own load_block / process_block lambdas, and
// attn_load_block reads `stream` and `rg` through references.  Both keep the compiler's schedule of the loops exactly as
// it was when each kernel carried its own copy (instruction for instruction, checked on the disassembly); direct calls, or
// the tail as a function, move instructions and registers in the streaming loop of dec_xrows_attn_kernel.

// the U K/V loads of one block of a stream (rows r0 + u * NS * 8 + stream * 8 + rg); a row index i >= lim is replaced by
// `clamp` so the loads are unconditional
template <int NS, int U, bool NT>
__device__ __forceinline__ void attn_load_block(const bf16_t *kb, const bf16_t *vb, int r0, const int &stream, const int &rg,
                                                int lim, int clamp, u32x4 (&kv)[U], u32x4 (&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int i = r0 + u * (NS * 8) + stream * 8 + rg;
        i = i < lim ? i : clamp;
        if (NT) {
            kv[u] = __builtin_nontemporal_load((const u32x4 *)(kb + (long)i * 64));
            vv[u] = __builtin_nontemporal_load((const u32x4 *)(vb + (long)i * 64));
        } else {
            kv[u] = *(const u32x4 *)(kb + (long)i * 64);
            vv[u] = *(const u32x4 *)(vb + (long)i * 64);
        }
    }
}

// every load of a block is IN FLIGHT before its first score is computed: the 2 U values pass through one empty asm, so
// nothing of the block can be consumed before all of it was requested (round 5: a re-ordered argument list was enough
// for the compiler to issue 6 of the 8 loads, start on the scores, and issue the last two afterwards -- 13.7 -> 16.5 us
// at 8 sequences: the stream is bound by bytes in flight per CU).  Not used by dec_xrows_attn_kernel: its fenced loop
// measured 1-3 % slower.
template <int U>
__device__ __forceinline__ void attn_block_fence(u32x4 (&kv)[U], u32x4 (&vv)[U]) {
    static_assert(U == 4, "attn_block_fence is written for 4 loads per block");
    asm volatile("" : "+v"(kv[0]), "+v"(kv[1]), "+v"(kv[2]), "+v"(kv[3]), "+v"(vv[0]), "+v"(vv[1]), "+v"(vv[2]), "+v"(vv[3]));
}

// one block of U x 8 rows of a stream: scores, block maximum, rescale, accumulate into the stream's running (m_run, l_run,
// oa).  qe: the query columns of this lane, pre-scaled.  Rows i >= n_keys score -1e30 and weigh 0.  MASK_V (the
// self-attention, whose loads are clamped to the cache's last row, not to the position): the V words of such a row are
// zeroed too -- they may hold anything, and 0 x NaN must not reach the sum.
template <int NS, int U, bool MASK_V>
__device__ __forceinline__ void attn_block(const float (&qe)[8], int r0, int stream, int rg, int n_keys, const u32x4 (&kv)[U],
                                           const u32x4 (&vv)[U], float &m_run, float &l_run, float (&oa)[8]) {
    float sc[U];
    float mb = -1e30f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = r0 + u * (NS * 8) + stream * 8 + rg;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a = __fmaf_rn(qe[2 * j], __uint_as_float(kv[u][j] << 16), a);
            a = __fmaf_rn(qe[2 * j + 1], __uint_as_float(kv[u][j] & 0xffff0000u), a);
        }
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        a += __shfl_xor(a, 4);
        sc[u] = i < n_keys ? a : -1e30f;
        mb = fmaxf(mb, sc[u]);
    }
    mb = fmaxf(mb, __shfl_xor(mb, 8));
    mb = fmaxf(mb, __shfl_xor(mb, 16));
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float m_new = fmaxf(m_run, mb);
    const float resc = __expf(m_run - m_new);  // 0 on the first block (m_run = -1e30), 1 when the max is unchanged
    l_run *= resc;
#pragma unroll
    for (int j = 0; j < 8; ++j) oa[j] *= resc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool live_row = sc[u] > -1e29f;
        const float pv = live_row ? __expf(sc[u] - m_new) : 0.f;
        l_run += pv;  // the 8 lanes of a row hold the same pv: only the row groups are summed (attn_stream_reduce)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned vw = (MASK_V && !live_row) ? 0u : vv[u][j];
            oa[2 * j] = __fmaf_rn(pv, __uint_as_float(vw << 16), oa[2 * j]);
            oa[2 * j + 1] = __fmaf_rn(pv, __uint_as_float(vw & 0xffff0000u), oa[2 * j + 1]);
        }
    }
    m_run = m_new;
}

// a stream's partials summed over its 8 row groups: every lane then holds the stream's l_run and its 8 output columns
__device__ __forceinline__ void attn_stream_reduce(float &l_run, float (&oa)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        oa[i] += __shfl_xor(oa[i], 8);
        oa[i] += __shfl_xor(oa[i], 16);
        oa[i] += __shfl_xor(oa[i], 32);
    }
    l_run += __shfl_xor(l_run, 8);
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
}

// ---- the ends of a stream, each stated once (which of the four attention kernels call which: DESIGN.md section 4)
// the eight query columns of a lane, scaled: hd^-0.5 (== hd^-0.25 on q and on k)
__device__ __forceinline__ void attn_scale_query(const float *qv, float (&qe)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) qe[i] = qv[i] * 0.125f;
}
// a reduced stream's partial (m, l, o[64]) to the 66 floats at `po` (HBM: dec_attn_combine_kernel merges them); row group 0
// holds it, lane e8 its columns e8 * 8 .. + 7
__device__ __forceinline__ void attn_store_partial(float *po, int rg, int e8, float m_run, float l_run, const float (&oa)[8]) {
    if (rg == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) po[2 + e8 * 8 + i] = oa[i];
        if (e8 == 0) {
            po[0] = m_run;
            po[1] = l_run;
        }
    }
}
// the same partial staged as stream w of the in-workgroup merge: wm[w], wl[w], wo[w][64]
__device__ __forceinline__ void attn_stage_partial(float *wm, float *wl, float *wo, int w, int rg, int e8, float m_run,
                                                   float l_run, const float (&oa)[8]) {
    if (rg == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wo[w * 64 + e8 * 8 + i] = oa[i];
        if (e8 == 0) {
            wm[w] = m_run;
            wl[w] = l_run;
        }
    }
}
// a workgroup behind the n_wg compute workgroups warms the L2 for the next GEMV's weights (l2_warm_tile); true: this was one
__device__ __forceinline__ bool attn_warm_up(int n_wg, const char *pf_ptr, long pf_tile_bytes, int nthreads) {
    if ((int)blockIdx.x < n_wg) return false;
    l2_warm_tile(pf_ptr, pf_tile_bytes, (int)blockIdx.x - n_wg, nthreads);
    return true;
}

// KERNEL ARGUMENTS / FIRST LOADS (round 5).  The round-4 kernel reached its first K/V load after six to seven DEPENDENT
// memory round trips (three lazy kernarg bursts, *n_live_ptr, *pos_ptr, live_rows[..], the query), each a cache miss on
// a fresh dispatch: 5.0 us for the ~1 MB self-attention of a batch of 8.  Now (a) the first 15 dwords of the argument
// list are everything the first loads need (small integers packed), so with -amdgpu-kernarg-preload-count=16 they are
// in SGPRs at the first instruction; (b) the position, the live count and the first pair's live row are requested
// TOGETHER, from always-valid addresses (a null pointer is replaced by `q`, the value discarded); (c) the query and the
// FIRST block of K/V rows of the first pair are requested before any of those values is needed: a self-attention row
// index is clamped to the cache's last row (T_stride - 1, an argument) instead of to the position, the rows past the
// position are masked as before and their V words zeroed (they may hold anything, and 0 x NaN must not reach the sum).
// The arithmetic -- blocks, order, merge -- is unchanged: same bits.
struct AttnCold {
    bf16_t *att;
    float *part;
    const char *pf_ptr;
    long pf_tile_bytes;
};
// RAGGED DECODE GROUPS (OFF, the self-attention only).  The rows of a group whose prompts differ in length are right-aligned:
// sequence b's first token sits at position off[b] of the group, so its keys are the cache rows [min(off[b], pos), pos].  The
// pair's K/V base pointers are advanced by that many rows and every row index below -- stream and block assignment, masks,
// merge order -- is RELATIVE to it: a row's bits are those of the same keys at the front of a cache with offset 0.  A
// sequence that has not started (pos < off[b]) attends to its one current row, which keeps it finite; nothing of it is kept.
// The offset is a load in FRONT of the speculative first block, which is why this is an instantiation of its own: uniform
// groups run the kernel they always ran.  Its pointer takes the place of `att` in the last preloaded dwords (14-15), and the
// first pair's offset is requested in the scalar burst for the row that pair has while every row is live (a group's whole
// prompt phase); only once the live list has been compacted does it cost a dependent load.
struct AttnColdOff {
    const int *off;   // [>= rows of the group]
    bf16_t *att;
    float *part;
    const char *pf_ptr;
    long pf_tile_bytes;
};
// TEACHER-FORCED PANELS (PANEL, the self-attention only).  The rows of a panel step are C windows x w consecutive positions
// of the SAME sequences: row r = c * w + s is position pos + s of window c.  Its pair reads the cache entry of WINDOW c (the
// step's QKV epilogue has just appended all w positions there) with pos + s + 1 keys; query and output are row r's.  Stream and
// block assignment, masks and merge order are functions of the key count only, so a row's bits are those of the uniform kernel
// at that position.  The speculative first block is clamped to the cache entry's last row as before (pos + s < T_stride).
// The width takes the place of `att` in the last preloaded dwords; uniform groups run the kernel they always ran.
struct AttnColdPanel {
    int w;
    bf16_t *att;
    float *part;
    const char *pf_ptr;
    long pf_tile_bytes;
};
// PROMPT PANELS (OFF and PANEL, wm_set_prompt_panel): a panel step over the prompt of a RAGGED group.  Row r = c * w + s is group
// position p = pos + s of window c: its cache entry is window c's, its keys are the cache rows [min(off[c], p), p] -- the base
// pointers advance by that offset and every row index is relative to it, so the row's bits are those of the OFF kernel at
// position p.  A row that has not started (p < off[c]) attends to its one current row, as there.  The speculative first block
// is clamped to the cache entry's last row (off[c] < T_stride, pos + s < T_stride).  An instantiation of its own.
struct AttnColdOffPanel {
    const int *off;   // [>= windows of the step]
    int w;
    bf16_t *att;
    float *part;
    const char *pf_ptr;
    long pf_tile_bytes;
};
template <bool OFF, bool PANEL> struct AttnColdSel { typedef AttnCold type; };
template <> struct AttnColdSel<true, false> { typedef AttnColdOff type; };
template <> struct AttnColdSel<false, true> { typedef AttnColdPanel type; };
template <> struct AttnColdSel<true, true> { typedef AttnColdOffPanel type; };
// (packA / packB / packC: packed by wm_pack_attn_rows / wm_pack_attn_keys, dec_launch.h)
template <int NS, int U, bool NT, bool DEEP = false, bool OFF = false, bool PANEL = false>
__global__ __launch_bounds__(DEEP ? 256 : NS * 64) void dec_rows_attn_kernel(
    const float *__restrict__ q, const bf16_t *__restrict__ kc, const bf16_t *__restrict__ vc,
    const int *__restrict__ pos_ptr, const int *__restrict__ live_rows /* [WM_DEC_MAXB] rows | [1] count, or null */,
    unsigned packA /* H | nsplit << 8 | flat_wpw << 16 */, unsigned packB /* T_stride | n_keys_const << 16 */,
    unsigned packC /* n_bh | n_wg << 16 */, typename AttnColdSel<OFF, PANEL>::type cold) {
    static_assert(!OFF || (NS == 4 && !DEEP), "row offsets: the causal self-attention only");
    static_assert(!PANEL || (NS == 4 && !DEEP), "panels: the causal self-attention only");
    const int H = (int)(packA & 0xffu), nsplit = (int)((packA >> 8) & 0xffu), flat_wpw = (int)(packA >> 16);
    const int T_stride = (int)(packB & 0xffffu), n_keys_const = (int)(packB >> 16);
    const int n_bh_full = (int)(packC & 0xffffu), n_wg = (int)(packC >> 16);
    const int d = H * 64;
    const int *n_live_ptr = live_rows ? live_rows + WM_DEC_MAXB : nullptr;
    constexpr bool SELF = NS == 4;  // the causal self-attention: the key count is the device-side position
    if (attn_warm_up(n_wg, cold.pf_ptr, cold.pf_tile_bytes, blockDim.x)) return;
    __shared__ float wm_[NS], wl_[NS];
    __shared__ float wo_[NS][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = lane >> 3, e8 = lane & 7;
    // FLAT launch (few pairs): the n_bh * NS (pair, stream) units are dealt to the waves of the grid one to one,
    // flat_wpw waves per workgroup, so that every CU streams an equal share whatever the pair count (B = 8 x 20 heads:
    // 1280 units = 256 workgroups of 5 waves); the waves of a workgroup are independent (partials to `part`, no barrier).
    int stream = (int)blockIdx.y * (NS / nsplit) + wave;  // blockDim.x == (NS / nsplit) * 64
    int bh0 = blockIdx.x, bh_step = n_wg;
    if (flat_wpw > 0) {
        const int unit = (int)blockIdx.x * flat_wpw + wave;
        if (unit >= n_bh_full * NS) return;  // wave-uniform
        bh0 = unit / NS;
        stream = unit % NS;
        bh_step = n_bh_full;  // one pair per wave
    }
    // ---- scalar burst: position, live count, the first pair's live row -- unconditional loads, valid addresses
    const int *dummy = (const int *)q;
    const int pos_raw = *(pos_ptr ? pos_ptr : dummy);
    const int nl_raw = *(n_live_ptr ? n_live_ptr : dummy);
    int off_raw = 0;
    if constexpr (OFF && !PANEL) off_raw = cold.off[bh0 / H];
    if constexpr (OFF && PANEL) off_raw = cold.off[(bh0 / H) / cold.w];   // the first pair's WINDOW
    // Early stop: sequences that have emitted <|endoftext|> (or used up their token budget) leave the decode group.
    // The arg-max kernel keeps a COMPACT list of the live rows; the pairs walked here are (live row, head), dealt to the
    // workgroups exactly like the full set, so the cache of a finished sequence is never read again and the remaining
    // pairs stay balanced over the chip.  (null: every row is live -- the fixed-length benchmark decode.)
    const int n_clamp = SELF ? T_stride - 1 : n_keys_const - 1;  // known without a load: the first block's row clamp
    auto load_block = [&](const bf16_t *kb, const bf16_t *vb, int r0, int clamp, u32x4 (&kv)[U], u32x4 (&vv)[U]) {
        attn_load_block<NS, U, NT>(kb, vb, r0, stream, rg, clamp, clamp, kv, vv);
    };
    bool first = true;
    int n_bh = n_bh_full, n_keys = n_keys_const;
    int pos_k = 0;  // OFF: the position, once known
    // n_wg <= n_bh workgroups (per split) walk the (sequence, head) pairs
    for (int pi = bh0; pi < n_bh; pi += bh_step) {
        if (flat_wpw == 0 && !first) __syncthreads();  // the previous pair's merge has been read
        const int h = pi % H;
        int b = pi / H;
        if (live_rows) b = live_rows[pi / H];  // first pair: pi < n_bh_full, a (possibly stale) valid row id
        const int bh = b * H + h;
        int bkv = bh;     // the pair's cache entry
        int ps = 0;       // PANEL: the row's position within the panel
        if constexpr (PANEL) {
            const int cw = b / cold.w;
            ps = b - cw * cold.w;
            bkv = cw * H + h;
        }
        const bf16_t *kb = kc + (long)bkv * T_stride * 64 + e8 * 8;
        const bf16_t *vb = vc + (long)bkv * T_stride * 64 + e8 * 8;
        const f32x4 *qp = (const f32x4 *)(q + (long)b * d + h * 64 + e8 * 8);
        const f32x4 q0 = qp[0], q1 = qp[1];
        int ob = 0;       // OFF: first cache row of this pair; row indices from here on are relative to it
        int clamp0 = first ? n_clamp : n_keys - 1 + ps;
        if constexpr (OFF && !PANEL) {
            if (first) {
                ob = b == bh0 / H ? off_raw : cold.off[b];   // (the position is not known yet: see below)
                clamp0 = n_clamp - ob;
            } else {
                ob = cold.off[b];
                ob = ob < pos_k ? ob : pos_k;
                clamp0 = pos_k - ob;
            }
            kb += (long)ob * 64;
            vb += (long)ob * 64;
        }
        if constexpr (OFF && PANEL) {   // the offset is the WINDOW's, the position the row's own: pos + ps
            if (first) {
                ob = b == bh0 / H ? off_raw : cold.off[b / cold.w];
                clamp0 = n_clamp - ob;
            } else {
                const int pk = pos_k + ps;
                ob = cold.off[b / cold.w];
                ob = ob < pk ? ob : pk;
                clamp0 = pk - ob;
            }
            kb += (long)ob * 64;
            vb += (long)ob * 64;
        }
        // SPEC: the first block (DEEP: every block) of this stream is requested BEFORE the position / live count / query is
        // looked at.  (This kernel serves the self-attention and the flat, deep cross-attention of a few pairs -- the latency
        // shapes; the streaming cross-attention is dec_xrows_attn_kernel, the round-4 loop.)
        constexpr bool SPEC = SELF || DEEP;
        constexpr int NB = DEEP ? ATT_MAXK / (NS * 8 * U) : 1;
        u32x4 kall[NB][U], vall[NB][U];
        if (SPEC) {
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
                load_block(kb, vb, blk * (NS * 8 * U), clamp0, kall[blk], vall[blk]);
        }
        if (first) {
            // (the empty asm ties the first USE of the two scalar loads to the arrival of the query: without it the
            // compiler hoists `pos + 1` in front of the loop and waits for the scalar loads before issuing the K/V loads)
            int pos_v = pos_raw, nl_v = nl_raw;
            if (SPEC) asm volatile("" : "+s"(pos_v), "+s"(nl_v) : "v"(q0[0]));
            if (n_live_ptr) n_bh = nl_v * H;
            if (pos_ptr) n_keys = pos_v + 1;
            first = false;
            if (pi >= n_bh) break;  // (workgroup- / wave-uniform) the speculative pair is not live
            if constexpr (OFF && !PANEL) {
                pos_k = n_keys - 1;
                if (pos_k < ob) {   // (workgroup-uniform) a sequence that has not started: its one key is the current row
                    kb -= (long)(ob - pos_k) * 64;
                    vb -= (long)(ob - pos_k) * 64;
                    ob = pos_k;
                    load_block(kb, vb, 0, 0, kall[0], vall[0]);
                }
            }
            if constexpr (OFF && PANEL) {
                pos_k = n_keys - 1;   // (the panel's first position; this row's is pos_k + ps)
                const int pk = pos_k + ps;
                if (pk < ob) {   // (workgroup-uniform) a row that has not started: its one key is its own current row
                    kb -= (long)(ob - pk) * 64;
                    vb -= (long)(ob - pk) * 64;
                    ob = pk;
                    load_block(kb, vb, 0, 0, kall[0], vall[0]);
                }
            }
        }
        int nk = n_keys;  // keys of this pair
        if constexpr (OFF) nk = pos_k + 1 - ob;
        if constexpr (PANEL) nk = n_keys + ps;
        if constexpr (OFF && PANEL) nk = pos_k + ps + 1 - ob;
        float qe[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qe[i] = q0[i] * 0.125f;  // hd^-0.5 (== hd^-0.25 on q and on k)
            qe[4 + i] = q1[i] * 0.125f;
        }
        float m_run = -1e30f, l_run = 0.f;
        float oa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto process_block = [&](int r0, const u32x4 (&kv)[U], const u32x4 (&vv)[U]) {
            attn_block<NS, U, SELF>(qe, r0, stream, rg, nk, kv, vv, m_run, l_run, oa);
        };
        if (DEEP) {
            // LATENCY shape (a handful of pairs: tiny.en single chunk = 48 waves on the whole chip): a stream's rows are
            // <= 6 blocks, and walking them one dependent memory round trip at a time was 9.2 us for 2.3 MB.  EVERY block
            // was requested above (48 x 16 B per lane); the same block arithmetic in the same order: same bits.
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
                if (blk * (NS * 8 * U) < nk) process_block(blk * (NS * 8 * U), kall[blk], vall[blk]);  // workgroup-uniform
        } else {
            if (SPEC) {
                attn_block_fence<U>(kall[0], vall[0]);
                process_block(0, kall[0], vall[0]);
            }
            for (int r0 = SPEC ? NS * 8 * U : 0; r0 < nk; r0 += NS * 8 * U) {  // workgroup-uniform trip count
                u32x4 kv[U], vv[U];
                load_block(kb, vb, r0, nk - 1, kv, vv);
                attn_block_fence<U>(kv, vv);
                process_block(r0, kv, vv);
            }
        }
        attn_stream_reduce(l_run, oa);
        if (nsplit > 1) {  // workgroup-uniform: the stream partials go to HBM, dec_attn_combine_kernel merges them
            attn_store_partial(cold.part + ((long)bh * NS + stream) * 66, rg, e8, m_run, l_run, oa);
            continue;
        }
        attn_stage_partial(wm_, wl_, &wo_[0][0], wave, rg, e8, m_run, l_run, oa);
        __syncthreads();
        if (tid < 64)  // head outputs feed the out-projection GEMV: stored in its fragment-tiled A-operand order
            cold.att[wm_tiled_offset((size_t)b, (size_t)(h * 64 + tid), (size_t)d)] = f2bf(attn_merge<NS>(wm_, wl_, &wo_[0][0], 64, tid));
    }
}

// The CROSS-attention family (NS = 8: streaming shape, flat deal, deep flat deal) keeps the round-4 loop: one unfenced
// block at a time, loads clamped to n_keys - 1.  Its block loop is the kernel that carries the roofline (66.8 us for 430 MB
// at 56 sequences), and every restructuring of it tried in round 5 -- peeled first block, fenced loads, asm-issued loads
// with counted waits -- left it 1-3 % slower (68.0 - 68.8 us) although the loads were in flight earlier: the compiler's
// schedule of THIS loop (packed FMAs across row groups, 196 instructions per block) is the one measured, and the shared
// block helpers above reproduce it instruction for instruction.  Only the argument list is the new one (hot scalars
// first, packed, preloaded); the key count of a cross-attention is an argument, so nothing here waits for the position.
// Of the stream-end helpers above it calls attn_scale_query alone: its warm-up return and its two partial stores stay spelled
// out because attn_warm_up, attn_store_partial and attn_stage_partial each change this kernel's instructions.
// (packA / packB / packC: packed by wm_pack_attn_rows / wm_pack_attn_keys, dec_launch.h)
template <int NS, int U, bool NT, bool DEEP = false>
__global__ __launch_bounds__(DEEP ? 256 : NS * 64) void dec_xrows_attn_kernel(
    const float *__restrict__ q, const bf16_t *__restrict__ kc, const bf16_t *__restrict__ vc,
    const int *__restrict__ pos_ptr, const int *__restrict__ live_rows /* [WM_DEC_MAXB] rows | [1] count, or null */,
    unsigned packA /* H | nsplit << 8 | flat_wpw << 16 */, unsigned packB /* T_stride | n_keys_const << 16 */,
    unsigned packC /* n_bh | n_wg << 16 */, AttnCold cold) {
    const int H = (int)(packA & 0xffu), nsplit = (int)((packA >> 8) & 0xffu), flat_wpw = (int)(packA >> 16);
    const int T_stride = (int)(packB & 0xffffu), n_keys_const = (int)(packB >> 16);
    int n_bh = (int)(packC & 0xffffu);
    const int n_wg = (int)(packC >> 16);
    const int d = H * 64;
    const int *n_live_ptr = live_rows ? live_rows + WM_DEC_MAXB : nullptr;
    bf16_t *att = cold.att;
    float *part = cold.part;
    const char *pf_ptr = cold.pf_ptr;
    const long pf_tile_bytes = cold.pf_tile_bytes;
    if ((int)blockIdx.x >= n_wg) {  // L2 warm-up workgroup for the next GEMV's weights
        l2_warm_tile(pf_ptr, pf_tile_bytes, (int)blockIdx.x - n_wg, blockDim.x);
        return;
    }
    // Early stop: sequences that have emitted <|endoftext|> (or used up their token budget) leave the decode group.
    // The arg-max kernel keeps a COMPACT list of the live rows; the pairs walked here are (live row, head), dealt to the
    // workgroups exactly like the full set, so the cache of a finished sequence is never read again and the remaining
    // pairs stay balanced over the chip.  (null: every row is live -- the fixed-length benchmark decode.)
    if (n_live_ptr) n_bh = *n_live_ptr * H;
    __shared__ float wm_[NS], wl_[NS];
    __shared__ float wo_[NS][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = lane >> 3, e8 = lane & 7;
    const int n_keys = pos_ptr ? (*pos_ptr + 1) : n_keys_const;
    const int last = n_keys - 1;
    // FLAT launch (few pairs): the n_bh * NS (pair, stream) units are dealt to the waves of the grid one to one,
    // flat_wpw waves per workgroup, so that every CU streams an equal share whatever the pair count (B = 8 x 20 heads:
    // 1280 units = 256 workgroups of 5 waves); the waves of a workgroup are independent (partials to `part`, no barrier).
    int stream = (int)blockIdx.y * (NS / nsplit) + wave;  // blockDim.x == (NS / nsplit) * 64
    int bh0 = blockIdx.x, bh_step = n_wg;
    if (flat_wpw > 0) {
        const int unit = (int)blockIdx.x * flat_wpw + wave;
        if (unit >= n_bh * NS) return;  // wave-uniform
        bh0 = unit / NS;
        stream = unit % NS;
        bh_step = n_bh;  // one pair per wave
    }
    // n_wg <= n_bh workgroups (per split) walk the (sequence, head) pairs
    for (int pi = bh0; pi < n_bh; pi += bh_step) {
        if (flat_wpw == 0 && pi != (int)blockIdx.x) __syncthreads();  // the previous pair's merge has been read
        const int h = pi % H;
        const int b = live_rows ? live_rows[pi / H] : pi / H;
        const int bh = b * H + h;
        const bf16_t *kb = kc + (long)bh * T_stride * 64 + e8 * 8;
        const bf16_t *vb = vc + (long)bh * T_stride * 64 + e8 * 8;
        float qe[8];
        attn_scale_query(q + (long)b * d + h * 64 + e8 * 8, qe);
        float m_run = -1e30f, l_run = 0.f;
        float oa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto load_block = [&](int r0, u32x4 (&kv)[U], u32x4 (&vv)[U]) {
            attn_load_block<NS, U, NT>(kb, vb, r0, stream, rg, n_keys, last, kv, vv);
        };
        auto process_block = [&](int r0, const u32x4 (&kv)[U], const u32x4 (&vv)[U]) {
            attn_block<NS, U, false>(qe, r0, stream, rg, n_keys, kv, vv, m_run, l_run, oa);
        };
        if (DEEP) {
            // LATENCY shape (a handful of pairs: tiny.en single chunk = 48 waves on the whole chip): a stream's rows are
            // <= 6 blocks, and walking them one dependent memory round trip at a time was 9.2 us for 2.3 MB.  Request
            // EVERY block first (48 x 16 B per lane), then run the same block arithmetic in the same order: same bits.
            constexpr int NB = ATT_MAXK / (NS * 8 * U);
            u32x4 kall[NB][U], vall[NB][U];
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) load_block(blk * (NS * 8 * U), kall[blk], vall[blk]);
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
                if (blk * (NS * 8 * U) < n_keys) process_block(blk * (NS * 8 * U), kall[blk], vall[blk]);  // workgroup-uniform
        } else {
            for (int r0 = 0; r0 < n_keys; r0 += NS * 8 * U) {  // workgroup-uniform trip count
                u32x4 kv[U], vv[U];
                load_block(r0, kv, vv);
                process_block(r0, kv, vv);
            }
        }
        attn_stream_reduce(l_run, oa);
        if (nsplit > 1) {  // workgroup-uniform: the stream partials go to HBM, dec_attn_combine_kernel merges them
            if (rg == 0) {
                float *po = part + ((long)bh * NS + stream) * 66;
#pragma unroll
                for (int i = 0; i < 8; ++i) po[2 + e8 * 8 + i] = oa[i];
                if (e8 == 0) {
                    po[0] = m_run;
                    po[1] = l_run;
                }
            }
            continue;
        }
        if (rg == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) wo_[wave][e8 * 8 + i] = oa[i];
            if (e8 == 0) {
                wm_[wave] = m_run;
                wl_[wave] = l_run;
            }
        }
        __syncthreads();
        if (tid < 64)  // head outputs feed the out-projection GEMV: stored in its fragment-tiled A-operand order
            att[wm_tiled_offset((size_t)b, (size_t)(h * 64 + tid), (size_t)d)] = f2bf(attn_merge<NS>(wm_, wl_, &wo_[0][0], 64, tid));
    }
}

// ------------------------------------------------------------------ cross-attention of CANDIDATE groups (best-of-N)
// A decode group of wm_transcribe_mel_best_of holds C windows x N candidates: row c * N + s is candidate s of window c, and
// the N rows of a window attend to ONE cross-K/V cache [C][H][T][64].  A stream of pair (window c, head h) requests every
// block of c's K/V once and runs attn_block on it for each LIVE candidate of c, each with its own (qe, m_run, l_run, oa):
// the stream geometry (NS = 8, U = 4, the block order), attn_stream_reduce and the merge (in LDS, or through `part` and
// dec_attn_combine_kernel) are those of dec_xrows_attn_kernel, so row c * N + s gets the bits the single-query kernel gives
// it over a copy of c's cache -- whatever N, the other rows and the launch shape.
// LIVE ROWS come from the compact ascending list the arg-max kernel maintains (rows of a window are adjacent in it).  Every
// wave reads the whole list with two vector loads per lane (<= 128 entries) and derives, by ballots alone, the number of live
// windows, the j-th live window (the pairs walked are (live window, head), dealt like dec_xrows_attn_kernel deals its pairs)
// and the N-bit mask of its live candidates: no LDS, no atomics and no scalar load beyond the live count in front of the
// first K/V load.  A window whose candidates have all finished is no pair any more: its cache is not read again.
// N is a template argument: the candidates' state lives in registers and the candidate loop is unrolled around wave-uniform
// branches (measured by the compiler: ~26 VGPRs per candidate, 114 / 162 / 188 / 214 / 240 for N = 1 .. 5).
// Shapes (wm_dec_attention_cand): one 8-wave workgroup per pair, <= one per CU, persistent (flat_wpw == 0, merge in LDS);
// or, below 256 pairs, the FLAT deal of the (pair, stream) units over ~256 workgroups (partials to `part`).
struct CandLive {
    int r_lo, r_hi;                      // this lane's list entries (lane, 64 + lane): row ids, -1 past the live count
    unsigned long long head_lo, head_hi; // entries that open a window
};
template <int N>
__device__ __forceinline__ void cand_window(const CandLive &L, int wj, int lane, int &c, unsigned &lm) {
    const int rank_lo = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(L.head_lo >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)L.head_lo, 0u));
    const int rank_hi = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(L.head_hi >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)L.head_hi, 0u)) +
                        __popcll(L.head_lo);
    const unsigned long long sel_lo = __ballot(((L.head_lo >> lane) & 1ull) && rank_lo == wj);
    const unsigned long long sel_hi = __ballot(((L.head_hi >> lane) & 1ull) && rank_hi == wj);
    int row;
    if (sel_lo) row = __builtin_amdgcn_readlane(L.r_lo, __builtin_ctzll(sel_lo));
    else row = __builtin_amdgcn_readlane(L.r_hi, sel_hi ? __builtin_ctzll(sel_hi) : 0);
    c = row / N;
    lm = 0u;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const int r = c * N + s;
        if ((__ballot(L.r_lo == r) | __ballot(L.r_hi == r)) != 0ull) lm |= 1u << s;
    }
}

// (packA / packB / packC: packed by wm_pack_attn_cand / wm_pack_attn_keys, dec_launch.h)
template <int N, bool NT>
__global__ __launch_bounds__(512) void dec_xcand_attn_kernel(
    const float *__restrict__ q, const bf16_t *__restrict__ kc, const bf16_t *__restrict__ vc,
    const int *__restrict__ live_rows /* [WM_DEC_MAXB] rows | [1] count, or null */, bf16_t *__restrict__ att,
    float *__restrict__ part, unsigned packA /* H | flat_wpw << 16 */, unsigned packB /* T_stride | n_keys << 16 */,
    unsigned packC /* C | n_wg << 16 */, const char *pf_ptr, long pf_tile_bytes) {
    // (the 15 dwords up to packC are everything the compute path reads: all of them arrive preloaded in SGPRs, and the only
    // scalar load in front of the first K/V load is the live count; pf_* are read by the warm-up workgroups alone)
    constexpr int NS = 8, U = 4;
    static_assert(N >= 1 && N <= 8, "1 .. 8 candidates per window");
    // Candidates held in registers at a time.  Five fit the 256 VGPRs two waves per SIMD leave a wave (240, no scratch);
    // six spill.  N = 6 .. 8 walk the window in TWO passes of (N + 1) / 2 candidates and request every block once per pass.
    constexpr int NP = N <= 5 ? N : (N + 1) / 2;
    const int H = (int)(packA & 0xffu), flat_wpw = (int)(packA >> 16);
    const int T_stride = (int)(packB & 0xffffu), n_keys = (int)(packB >> 16);
    const int C = (int)(packC & 0xffffu), n_wg = (int)(packC >> 16);
    const int d = H * 64;
    if (attn_warm_up(n_wg, pf_ptr, pf_tile_bytes, blockDim.x)) return;
    __shared__ float wm_[N][NS], wl_[N][NS];
    __shared__ float wo_[N][NS][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = lane >> 3, e8 = lane & 7;
    const int last = n_keys - 1;
    // ---- the live list -> windows (every wave for itself; null: every row of the C windows is live)
    CandLive L;
    {
        int n_live = C * N, p_lo = lane - 1, p_hi = lane + 63;
        L.r_lo = lane;
        L.r_hi = lane + 64;
        if (live_rows) {
            n_live = live_rows[WM_DEC_MAXB];
            L.r_lo = live_rows[lane];
            L.r_hi = live_rows[lane + 64];
            p_lo = live_rows[lane > 0 ? lane - 1 : 0];
            p_hi = live_rows[lane + 63];
        }
        const bool v_lo = lane < n_live, v_hi = lane + 64 < n_live;
        L.r_lo = v_lo ? L.r_lo : -1;
        L.r_hi = v_hi ? L.r_hi : -1;
        L.head_lo = __ballot(v_lo && (lane == 0 || p_lo / N != L.r_lo / N));
        L.head_hi = __ballot(v_hi && p_hi / N != L.r_hi / N);
    }
    const int n_pairs = (__popcll(L.head_lo) + __popcll(L.head_hi)) * H;   // (live window, head)
    int stream = wave;  // flat_wpw == 0: blockDim.x == NS * 64
    int p0 = blockIdx.x, p_step = n_wg;
    if (flat_wpw > 0) {   // FLAT launch: the n_pairs * NS (pair, stream) units dealt to the waves of the grid one to one
        const int unit = (int)blockIdx.x * flat_wpw + wave;
        if (unit >= n_pairs * NS) return;  // wave-uniform
        p0 = unit / NS;
        stream = unit % NS;
        p_step = n_pairs;  // one pair per wave
    }
    for (int pi = p0; pi < n_pairs; pi += p_step) {
        if (flat_wpw == 0 && pi != (int)blockIdx.x) __syncthreads();  // the previous pair's merge has been read
        const int h = pi % H;
        int c;
        unsigned lm;   // bit s: candidate s of window c is live (wave-uniform)
        cand_window<N>(L, pi / H, lane, c, lm);
        const int ch = c * H + h;
        const bf16_t *kb = kc + (long)ch * T_stride * 64 + e8 * 8;
        const bf16_t *vb = vc + (long)ch * T_stride * 64 + e8 * 8;
        // the candidates of the window, NP at a time in registers (N <= 5: one pass)
        for (int s0 = 0; s0 < N; s0 += NP) {
            const unsigned pm = (lm >> s0) & ((1u << NP) - 1u);   // live candidates of this pass (wave-uniform)
            if (NP < N && pm == 0u) continue;
            float qe[NP][8], m_run[NP], l_run[NP], oa[NP][8];
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                m_run[s] = -1e30f;
                l_run[s] = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    qe[s][i] = 0.f;
                    oa[s][i] = 0.f;
                }
                if ((pm >> s) & 1u) attn_scale_query(q + (long)(c * N + s0 + s) * d + h * 64 + e8 * 8, qe[s]);
            }
            for (int r0 = 0; r0 < n_keys; r0 += NS * 8 * U) {  // workgroup-uniform trip count
                u32x4 kv[U], vv[U];
                attn_load_block<NS, U, NT>(kb, vb, r0, stream, rg, n_keys, last, kv, vv);
#pragma unroll
                for (int s = 0; s < NP; ++s)
                    if ((pm >> s) & 1u) attn_block<NS, U, false>(qe[s], r0, stream, rg, n_keys, kv, vv, m_run[s], l_run[s], oa[s]);
            }
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                if (!((pm >> s) & 1u)) continue;   // wave-uniform
                attn_stream_reduce(l_run[s], oa[s]);
                if (rg != 0) continue;
                if (flat_wpw > 0)  // the stream partials go to HBM, dec_attn_combine_kernel merges them
                    attn_store_partial(part + ((long)((c * N + s0 + s) * H + h) * NS + stream) * 66, rg, e8, m_run[s], l_run[s], oa[s]);
                else
                    attn_stage_partial(wm_[s0 + s], wl_[s0 + s], &wo_[s0 + s][0][0], wave, rg, e8, m_run[s], l_run[s], oa[s]);
            }
        }
        if (flat_wpw > 0) continue;
        __syncthreads();
        // wave s merges candidate s: head outputs in the out-projection GEMV's fragment-tiled A-operand order
        if (wave < N && ((lm >> wave) & 1u))
            att[wm_tiled_offset((size_t)(c * N + wave), (size_t)(h * 64 + lane), (size_t)d)] =
                f2bf(attn_merge<NS>(wm_[wave], wl_[wave], &wo_[wave][0][0], 64, lane));
    }
}


// ------------------------------------------------------------------ fused query projection + cross-attention
// LATENCY shape of a decoder layer's cross-attention (round 5): 96 .. 256 (sequence, head) pairs -- a batch of 5 .. 12 at 20
// heads -- and nothing else decoding on the device.  There the cross_attn_ln + query GEMV is a 3.6 us launch that does
// 0.8 us of streaming, and its only consumer is the attention kernel behind it.  This kernel is both: the workgroup of
// pair (b, h) first forms ITS OWN 64 query values -- the four 16-row weight tiles of head h, multiplied with the block of
// 16 residual rows that holds b, K split over the waves exactly as dec_gemv_kernel splits it, partials summed through LDS
// in part order, LayerNorm fold applied by the very functions the GEMV uses (gemv_unit_load / gemv_unit_stats): the 64
// values are bit for bit what the GEMV would have left in HBM -- while the first block of its K/V rows is already on its
// way, then walks its six blocks like the streaming kernel (attn_block / attn_stream_reduce, same order: same
// bits).  One launch and one kernel boundary less per layer.  Workgroup -> pair: the head-major pair list is cut into 8
// equal ranges, one per XCD (workgroup id % 8, observed placement), so every XCD streams the same number of caches and a
// head's 164 KB weight slice crosses the fabric once or twice and is an L2 hit for the other sequences of the head; the
// L2 warm-up workgroups of the previous launch place the tiles the same way (pf_head_major).  (A first version put head h
// on XCD h % 8: 24 vs 16 workgroups per XCD at 20 heads x 8, and the stream ran at the pace of the fuller XCDs.)
// "Bit-identical to the two launches" is a statement about LIVE rows.  With early stop on, only workgroups of live pairs get
// past the `bi >= n_live` return, so (a) the rows' new LayerNorm means (mean_out) are written by the head-0 workgroups of the
// 16-row blocks that still hold a live row -- a block whose rows are all finished keeps the means of two LayerNorms earlier --
// and (b) the query itself never reaches HBM (m->dq is not written by the fused launch).  Finished rows' tokens are fixed
// already (pad_tok) and nothing reads their residual again; tests/test_model_gpu.py checks the fused shape against the two
// launches with early stop on at 8 rows (one block) and at 24 rows of 8 heads (two blocks, blk > 0).
struct FqCold {
    const float *c1, *c2, *stats_in, *mean_in;
    float *mean_out;
    bf16_t *att;
    long stats_stride;
    int K, N;
    const char *pf_ptr;    // L2 warm-up of the NEXT launch's weights by extra workgroups (as in dec_rows_attn_kernel)
    long pf_tile_bytes;
    int n_wg;              // compute workgroups; ids beyond are warm-up workgroups
};
// (packA / packB: packed by wm_pack_attn_fq / wm_pack_attn_keys, dec_launch.h)
template <int SPW, bool NT>
__global__ __launch_bounds__(512) void dec_xattn_fq_kernel(const bf16_t *__restrict__ Wq, const bf16_t *__restrict__ xb,
                                                           const bf16_t *__restrict__ kc, const bf16_t *__restrict__ vc,
                                                           const int *__restrict__ live_rows, unsigned packA /* H | B << 8 */,
                                                           unsigned packB /* T_stride | n_keys << 16 */, int K, FqCold cold) {
    constexpr int NS = 8, U = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = (int)(packA & 0xffu), B = (int)(packA >> 8);
    const int T_stride = (int)(packB & 0xffffu), n_keys = (int)(packB >> 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = lane >> 3, e8 = lane & 7;
    // workgroup -> (head, sequence): residue r = id % 8 is the XCD; the heads r, r + 8, r + 16 live there
    if (attn_warm_up(cold.n_wg, cold.pf_ptr, cold.pf_tile_bytes, 512)) return;
    // workgroup -> pair: the head-major pair list (h, b) is cut into 8 equal ranges, one per XCD (id % 8, observed
    // placement): every XCD streams the same number of caches and hosts 2 - 4 heads' weight slices
    const int per = (H * B + 7) >> 3;
    const int pidx = ((int)blockIdx.x >> 3) + per * ((int)blockIdx.x & 7);
    if (((int)blockIdx.x >> 3) >= per || pidx >= H * B) return;  // workgroup-uniform
    const int h = pidx / B, bi = pidx % B;
    int n_live = B;
    if (live_rows) n_live = live_rows[WM_DEC_MAXB];
    int b = bi;
    if (live_rows) b = live_rows[bi];  // (bi < B: a possibly stale, valid row id; discarded below when bi >= n_live)
    const int NP = (K >> 5) / SPW;     // K parts == waves that multiply (<= 8)
    const int blk = b >> 4, bl = b & 15;
    float *red = (float *)smem;                    // [NP][4 tiles][64][4]
    float *stbase = red + NP * 4 * 256;            // [4][32] statistics slots, one per tile wave
    float *q_lds = stbase + 4 * 32;                // [64]
    // ---- every load in flight: the head's weight tiles and the residual block (waves < NP) ...
    u32x4 wf[4][SPW], af[SPW];
    if (wave < NP) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bf16_t *wp = Wq + (((long)(h * 4 + t) * (K >> 5) + (long)wave * SPW) * 64 + lane) * 8;
#pragma unroll
            for (int u = 0; u < SPW; ++u) wf[t][u] = *(const u32x4 *)(wp + u * 512);
        }
        const bf16_t *ap = xb + (((long)blk * (K >> 5) + (long)wave * SPW) * 64 + lane) * 8;
#pragma unroll
        for (int u = 0; u < SPW; ++u) af[u] = *(const u32x4 *)(ap + u * 512);
    }
    // ... the LayerNorm operands of the tile this wave will finish (waves 0 .. 3: tile h * 4 + wave) ...
    DecGemvDev p = {};
    p.B = B; p.N = cold.N; p.K = K; p.c1 = cold.c1; p.c2 = cold.c2; p.stats_in = cold.stats_in;
    p.stats_stride = cold.stats_stride; p.mean_in = cold.mean_in; p.mean_out = cold.mean_out;
    p.out_f32 = nullptr; p.ts.rng = nullptr;
    GemvUnitOps<DE_Q, true> ops;
    const int my_tile = h * 4 + (wave & 3);
    if (wave < 4) gemv_unit_load<DE_Q, true>(p, ops, my_tile, blk * 16, lane, 0, 4, true);
    // ... and the first block of this stream's K/V rows (stream = wave)
    const int stream = wave;
    const int bh = b * H + h;
    const bf16_t *kb = kc + (long)bh * T_stride * 64 + e8 * 8;
    const bf16_t *vb = vc + (long)bh * T_stride * 64 + e8 * 8;
    auto load_block = [&](int r0, u32x4 (&kv)[U], u32x4 (&vv)[U]) {
        attn_load_block<NS, U, NT>(kb, vb, r0, stream, rg, n_keys - 1, n_keys - 1, kv, vv);
    };
    u32x4 kv0[U], vv0[U];
    load_block(0, kv0, vv0);
    if (bi >= n_live) return;  // (workgroup-uniform) the speculative pair is not live
    // ---- the query: products of this wave's K part, split-K sum through LDS in part order, LayerNorm fold
    if (wave < NP) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < SPW; ++u)
                a4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[u]), __builtin_bit_cast(bf16x8, wf[t][u]), a4, 0, 0, 0);
            *(f32x4 *)(red + ((wave * 4 + t) * 64 + lane) * 4) = a4;
        }
    }
    if (wave < 4) gemv_unit_stats<DE_Q, true>(p, ops, stbase + wave * 32, lane, my_tile, blk * 16);
    __syncthreads();
    if (wave < 4) {
        f32x4 sum = *(const f32x4 *)(red + ((0 * 4 + wave) * 64 + lane) * 4);
        for (int w = 1; w < NP; ++w) sum += *(const f32x4 *)(red + ((w * 4 + wave) * 64 + lane) * 4);
        const float2 ms = *(const float2 *)(stbase + wave * 32 + bl * 2);
        const int kq = lane >> 4, nrow = lane & 15;
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (kq * 4 + r == bl) v = __fmaf_rn(ms.x, sum[r], __fmaf_rn(ms.y, ops.c1v, ops.c2v));  // == gemv_unit_epilogue (LN)
        if (kq == (bl >> 2)) q_lds[wave * 16 + nrow] = v;
    }
    __syncthreads();
    float qe[8];
    attn_scale_query(q_lds + e8 * 8, qe);
    // ---- the stream, block by block: the shared block arithmetic (attn_block)
    float m_run = -1e30f, l_run = 0.f;
    float oa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto process_block = [&](int r0, const u32x4 (&kv)[U], const u32x4 (&vv)[U]) {
        attn_block<NS, U, false>(qe, r0, stream, rg, n_keys, kv, vv, m_run, l_run, oa);
    };
    process_block(0, kv0, vv0);
    for (int r0 = NS * 8 * U; r0 < n_keys; r0 += NS * 8 * U) {  // workgroup-uniform trip count
        u32x4 kv[U], vv[U];
        load_block(r0, kv, vv);
        attn_block_fence<U>(kv, vv);
        process_block(r0, kv, vv);
    }
    attn_stream_reduce(l_run, oa);
    float *wm_ = red, *wl_ = red + NS, *wo_ = red + 2 * NS;  // (the split-K partials are dead: both barriers passed)
    __syncthreads();
    attn_stage_partial(wm_, wl_, wo_, wave, rg, e8, m_run, l_run, oa);
    __syncthreads();
    if (tid < 64)
        cold.att[wm_tiled_offset((size_t)b, (size_t)(h * 64 + tid), (size_t)(H * 64))] = f2bf(attn_merge<NS>(wm_, wl_, wo_, 64, tid));
}

// Merge the NS stream partials of every pair -> bf16 head outputs (same arithmetic as the in-kernel merge).
// grid B*H, 64 threads.
template <int NS>
__global__ __launch_bounds__(64) void dec_attn_combine_kernel(const float *__restrict__ part, int H, int d,
                                                              bf16_t *__restrict__ att) {
    __shared__ float wm_[NS], wl_[NS];
    const int bh = blockIdx.x, b = bh / H, h = bh % H, e = threadIdx.x;
    const float *pp = part + (long)bh * NS * 66;
    float oo[NS], mm[NS], ll[NS];
#pragma unroll
    for (int w = 0; w < NS; ++w) oo[w] = pp[2 + w * 66 + e];  // requested together with (m, l): ONE memory round trip
    if (e < NS) {
        wm_[e] = pp[e * 66];
        wl_[e] = pp[e * 66 + 1];
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        mm[w] = wm_[w];
        ll[w] = wl_[w];
    }
    att[wm_tiled_offset((size_t)b, (size_t)(h * 64 + e), (size_t)d)] = f2bf(attn_merge_core<NS>(mm, ll, oo));
}

// ------------------------------------------------------------------ arg-max -> next token
// ONE workgroup of 16 waves closes a decode step: wave b reduces the per-tile packed maxima of
// sequence b (all loads in flight at once), the chosen token goes into the sequence buffer at
// position pos+1 unless that position belongs to the prompt, then the SAME launch embeds the
// tokens of position pos+1 (token + positional embedding, plus the LayerNorm partial statistics
// the next layer-0 GEMV expects) and advances the device-side position -- so a step has no
// separate embedding launch and *pos_ptr has exactly one writer.
// X (wm_transcribe's extended decode, WmXDev): the same close, plus the log-prob of the chosen token under the filtered
// distribution, no_speech_prob at the <|startoftranscript|> position, and -- under sampling -- the sum rule decided on
// the raw text maximum.  The (max, sum exp) partials of a row are merged over 16 FIXED tile segments (any participant
// count P scans whole segments; each segment and the final merge have one summation order): the bits do not depend on
// the rows per workgroup, i.e. on the decode group.
template <bool X>
__device__ __forceinline__ void argmax_embed_body(const unsigned long long *__restrict__ tilemax,
                                                  int n_tiles, int B, int *__restrict__ seq,
                                                  int *__restrict__ pos_ptr, int n_prompt,
                                                  int *__restrict__ result, int arg_first,
                                                  const bf16_t *__restrict__ emb,
                                                  const float *__restrict__ pemb, int d, int n_ctx,
                                                  float *__restrict__ x, bf16_t *__restrict__ xb,
                                                  float *__restrict__ stats_out, const WmTsDev &ts,
                                                  int *__restrict__ arrive, int fallback_tok,
                                                  float *__restrict__ mean_buf, const WmStopDev &stop, int rpw,
                                                  const WmXDev &xd, const int *__restrict__ off) {
    __shared__ int tok_s[16];
    __shared__ int is_last_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the position is requested now and first USED after the per-tile maxima have been requested (the empty asm below
    // ties its use to the first of them): the round-4 kernel waited for it before issuing a single load
    const int pos_raw = *(pos_ptr ? pos_ptr : (const int *)tilemax);
    int pos = 0;
    const int bw = blockIdx.x * rpw;  // this workgroup's rows (rpw <= 16): one per wave (the row's OWNER: wave r owns row bw + r)
    // Round 5: the waves that own no row HELP.  A row's 3 242 per-tile keys were one wave's work -- seven dependent round
    // trips of 8 x 64 keys (one sequence: 15 of the 16 waves idle, ~5 us of the step's tail) -- now the row's P = 1 +
    // (16 - rows) / rows participants take a contiguous share each (one sequence: 16 x 203 keys = ONE trip) and the owner
    // takes the maximum of their partial maxima (a maximum: any order, same bits).
    __shared__ unsigned long long part_s[16][16];
    const int nrows = B - bw < rpw ? B - bw : rpw;
    const int hpr = (16 - nrows) / nrows;                 // helpers per row
    const int P = 1 + hpr;
    int my_row = -1, my_pi = 0;                           // the row this wave scans for, and its participant index
    if (wave < nrows) { my_row = wave; }
    else if (wave - nrows < hpr * nrows) { my_row = (wave - nrows) % nrows; my_pi = 1 + (wave - nrows) / nrows; }
    if (my_row >= 0) {  // wave-uniform
        const unsigned long long *row = tilemax + (long)(bw + my_row) * n_tiles;
        const int chunk = (n_tiles + P - 1) / P, t_lo = my_pi * chunk, t_hi = t_lo + chunk < n_tiles ? t_lo + chunk : n_tiles;
        unsigned long long key = 0ull;
        for (int t0 = t_lo + lane; t0 < t_hi; t0 += 64 * 8) {
            unsigned long long k[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + 64 * u;
                k[u] = row[t < t_hi ? t : t0];  // clamped: duplicates do not change a max
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) key = k[u] > key ? k[u] : key;
        }
        key = key_max_xor<64>(key);
        if (lane == 0) part_s[my_row][my_pi] = key;
    }
    __shared__ float seg_s[X ? 16 : 1][X ? 16 : 1][4];   // [row][segment]: allowed text (m, s), unfiltered (m, s)
    if (X && my_row >= 0) {  // wave-uniform
        lse_row_segments(xd, (long)(bw + my_row) * n_tiles, n_tiles, pos_raw == xd.par->sot_pos, my_pi, P, lane, seg_s[my_row]);
    }
    __syncthreads();
    for (int b = bw + wave; b < B && b < bw + nrows; b += 16) {  // wave-uniform, at most one trip: the owners
        unsigned long long key = lane < P ? part_s[wave][lane] : 0ull;
        {
            int pv = pos_raw;
            asm volatile("" : "+s"(pv) : "v"((unsigned)key));
            pos = pos_ptr ? pv : 0;
        }
        key = __shfl(key_max_xor<16>(key), 0);   // P <= 16 partial maxima in lanes 0 .. 15; every lane of the owner carries the row's key
        Lse lt{-1e30f, 0.f}, la{-1e30f, 0.f};
        if (X) lse_row_total(seg_s[wave], lane, lt, la);   // the row's 16 segments, in a fixed order
        // `key` is the best allowed TEXT token; the decision against the timestamps (X: the key may be a perturbed score)
        const RowChoice ch = row_choose(ts, b, n_tiles, lane, key, X ? lt.m : argmax_key_value(key));
        if (lane == 0) {
            // ch.key == 0: nothing admissible: never index with -1
            int tok = ch.key ? argmax_key_index(ch.key) : fallback_tok;
            if (X && pos + 1 >= n_prompt) {
                float lp = row_logprob(ts, xd, b, n_tiles, ch, lt);
                if (stop.done && stop.done[b]) lp = 0.f;   // finished earlier: nothing is generated here
                xd.logprob[(long)(pos + 1 - n_prompt) * B + b] = lp;
            }
            if (X && pos == xd.par->sot_pos) xd.nospeech[b] = row_no_speech(xd, b, la);
            if (stop.done && pos + 1 >= n_prompt) {
                // the token at index pos + 1 is generated token number gi (0-based)
                const int gi = pos + 1 - n_prompt;
                if (stop.done[b]) {
                    tok = stop.pad_tok;                        // finished earlier: padding (the host truncates at the length)
                } else if ((stop.eot >= 0 && tok == stop.eot) || (stop.budget && gi + 1 >= stop.budget[b])) {
                    stop.done[b] = 1;                          // this token is the row's last
                }
            }
            if (ts.rng && pos + 1 >= n_prompt) {
                // the token at index pos + 1 was sampled: advance the history and derive the ranges of the next position
                *(int4 *)(ts.rng + b * 4) = ts_advance(ts, ts.hist + b * 4, tok);
            }
            int nxt = tok;
            if (seq) {
                if (pos + 1 >= n_prompt) seq[(pos + 1) * B + b] = tok;
                else nxt = seq[(pos + 1) * B + b];
            }
            tok_s[b - bw] = nxt;
            if (result) result[b] = tok - arg_first;
        }
    }
    __syncthreads();
    {   // (waves without a row of their own have not looked at the position yet)
        int pv = pos_raw;
        asm volatile("" : "+s"(pv));
        pos = pos_ptr ? pv : 0;
    }
    if (x && pos + 1 < n_ctx) {
        for (int b = bw + wave; b < B && b < bw + nrows; b += 16) {
            const long tok = tok_s[b - bw];
            // a ragged group (off != null): row b's prompt starts at position off[b], its positional row counts from there
            const int prow = off ? max(pos + 1 - off[b], 0) : pos + 1;
            embed_row(tok, prow, b, lane, emb, pemb, d, x, xb, stats_out, mean_buf);
        }
    }
    // *pos_ptr has ONE writer: the last workgroup to arrive (every workgroup read the position before it arrived)
    __syncthreads();
    if (!stop.done) {
        if (threadIdx.x == 0 && pos_ptr) {
            if (gridDim.x == 1) {
                *pos_ptr = pos + 1;
            } else if (atomicAdd(arrive, 1) == (int)gridDim.x - 1) {
                *arrive = 0;
                *pos_ptr = pos + 1;
            }
        }
        return;
    }
    // early stop on: the last workgroup to arrive also rebuilds the compact list of live rows from every workgroup's
    // done flags (release fence before arriving, acquire fence after: the flags were written by other CUs / XCDs)
    if (threadIdx.x == 0) {
        int last = 1;
        if (gridDim.x > 1) {
            __threadfence();
            last = atomicAdd(arrive, 1) == (int)gridDim.x - 1;
            if (last) {
                *arrive = 0;
                __threadfence();
            }
        }
        is_last_s = last;
    }
    __syncthreads();
    if (is_last_s && wave == 0) {
        live_list_rebuild(stop, B, lane,
                          [&](int b) { return __hip_atomic_load(stop.done + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0; });
        if (lane == 0 && pos_ptr) *pos_ptr = pos + 1;
    }
}

__global__ __launch_bounds__(1024) void argmax_embed_kernel(const unsigned long long *__restrict__ tilemax,
                                                             int n_tiles, int B, int *__restrict__ seq,
                                                             int *__restrict__ pos_ptr, int n_prompt,
                                                             int *__restrict__ result, int arg_first,
                                                             const bf16_t *__restrict__ emb,
                                                             const float *__restrict__ pemb, int d, int n_ctx,
                                                             float *__restrict__ x, bf16_t *__restrict__ xb,
                                                             float *__restrict__ stats_out, WmTsDev ts,
                                                             int *__restrict__ arrive, int fallback_tok,
                                                             float *__restrict__ mean_buf, WmStopDev stop, int rpw,
                                                             const int *__restrict__ off) {
    const WmXDev none = {};
    argmax_embed_body<false>(tilemax, n_tiles, B, seq, pos_ptr, n_prompt, result, arg_first, emb, pemb, d, n_ctx, x, xb,
                             stats_out, ts, arrive, fallback_tok, mean_buf, stop, rpw, none, off);
}
__global__ __launch_bounds__(1024) void argmax_embed_x_kernel(const unsigned long long *__restrict__ tilemax,
                                                               int n_tiles, int B, int *__restrict__ seq,
                                                               int *__restrict__ pos_ptr, int n_prompt,
                                                               int *__restrict__ result, int arg_first,
                                                               const bf16_t *__restrict__ emb,
                                                               const float *__restrict__ pemb, int d, int n_ctx,
                                                               float *__restrict__ x, bf16_t *__restrict__ xb,
                                                               float *__restrict__ stats_out, WmTsDev ts,
                                                               int *__restrict__ arrive, int fallback_tok,
                                                               float *__restrict__ mean_buf, WmStopDev stop, int rpw,
                                                               WmXDev xd, const int *__restrict__ off) {
    argmax_embed_body<true>(tilemax, n_tiles, B, seq, pos_ptr, n_prompt, result, arg_first, emb, pemb, d, n_ctx, x, xb,
                            stats_out, ts, arrive, fallback_tok, mean_buf, stop, rpw, xd, off);
}

// the DE_LOGITS_X epilogue's Gumbel noise for a range of ids (test hook)
__global__ void sample_noise_kernel(unsigned long long seed, int chunk, int gi, int n0, int count, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = wm_gumbel_from_bits(wm_sample_bits(seed, (unsigned)chunk, (unsigned)gi, (unsigned)(n0 + i)));
}

// start of a decode: nobody is done, every row is live
__global__ void dec_live_init_kernel(WmStopDev stop, int B) {
    const int b = threadIdx.x;
    if (b < B) {
        stop.done[b] = 0;
        stop.live_rows[b] = b;
    }
    if (b == 0) *stop.n_live = B;
}

// ------------------------------------------------------------------ synthetic weights ----
// Mirrors weights.synthetic_values(): Irwin-Hall(4) of 16-bit hash words, exact integer sum,
// one f32 multiply, optional bf16 rounding -> bit-identical to the numpy generator.
__device__ __forceinline__ unsigned hash32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(256) void synth_fill_kernel(void *dst, int is_bf16, size_t n, unsigned key,
                                                         float scale, int layout, int conv_c, int kpad,
                                                         int kind, float gain) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v;
        if (kind == 2) {
            v = 1.0f;
        } else if (kind == 3) {
            v = 0.0f;
        } else {
            const unsigned h1 = hash32((unsigned)i ^ key);
            const unsigned h2 = hash32(h1 + 0x85ebca6bu);
            const int s = (int)(h1 & 0xffffu) + (int)(h1 >> 16) + (int)(h2 & 0xffffu) + (int)(h2 >> 16);
            v = __fmul_rn(__fmul_rn((float)(s - 131070), scale), gain);  // two roundings, as on the host
        }
        size_t o = i;
        if (layout == WL_CONV) {
            const size_t per = (size_t)conv_c * 3;
            const size_t oc = i / per, rem = i % per, c = rem / 3, tap = rem % 3;
            o = oc * kpad + tap * conv_c + c;
        } else if (layout == WL_TILED) {
            o = wm_tiled_offset(i / (size_t)kpad, i % (size_t)kpad, (size_t)kpad);
        }
        if (is_bf16)
            ((bf16_t *)dst)[o] = f2bf(v);
        else
            ((float *)dst)[o] = (kind == 0) ? bf2f(f2bf(v)) : v;  // matrices are bf16-representable everywhere
    }
}

#define GEMV_ARGS(p) (p).W, (p).a, (p).pos_ptr, (p).c2, (p).K, (p).n_tiles, (p).B, (p).bgroups, (p).n_tg, (p).n_tg_pad, (p).out_f32, (p)
// The plan (wm_plan_gemv) has chosen and checked the shape; here it is mapped to the kernel instantiation.  The TWO / RESID /
// WIDE guards keep the set of instantiations to the shapes a plan can ask for.
template <int SPW, int EPI, bool LN>
int launch_gemv_shape(wm_ctx *ctx, const DecGemvDev &p, const DecGemvPlan &pl) {
    hipStream_t s = ctx->stream;
    const int tn = pl.tn, nblk = pl.nblk, grid = pl.grid, th = pl.block;
    const size_t lds = (size_t)pl.lds;
    constexpr bool TWO = !LN && EPI == DE_RESID && SPW >= 6 && SPW <= 10;
    constexpr bool RESID = !LN && EPI == DE_RESID;
    constexpr bool LOGITS = de_is_logits(EPI);
    constexpr bool WIDE = LN && (de_is_qkv(EPI) || EPI == DE_GELU || LOGITS) && SPW <= 6;
    if (pl.ppw == 2 && TWO) {  // 16 K parts on 8 waves (the K = 4d residual products at more than one batch block)
        if (nblk == 2) dec_gemv_kernel<TWO ? SPW : 6, 1, 2, TWO ? EPI : DE_RESID, TWO ? LN : false, 2, 4><<<grid, th, lds, s>>>(GEMV_ARGS(p));
        else if (pl.row_split) dec_gemv_kernel<TWO ? SPW : 6, 1, 1, TWO ? EPI : DE_RESID, TWO ? LN : false, 2, 4><<<grid, th, lds, s>>>(GEMV_ARGS(p));
        else dec_gemv_kernel<TWO ? SPW : 6, 1, 1, TWO ? EPI : DE_RESID, TWO ? LN : false, 2><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    } else if (pl.ppw == 1 && pl.row_split && RESID && nblk == 1) {   // four waves per (tile, block) unit
        dec_gemv_kernel<SPW, 1, 1, RESID ? EPI : DE_RESID, RESID ? LN : false, 1, 4><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    } else if (pl.ppw == 1 && pl.row_split && RESID && nblk == 2 && SPW <= 8) {
        dec_gemv_kernel<SPW <= 8 ? SPW : 2, 1, 2, RESID ? EPI : DE_RESID, RESID ? LN : false, 1, 4><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    } else if (pl.ppw != 1 || pl.row_split) {
        wm_set_error("dec_gemv: no kernel for the planned shape (ppw %d, row split %d, nblk %d, spw %d)", pl.ppw, pl.row_split, nblk, SPW);
        return WM_ERR_INVALID;
    }
    else if (tn == 1 && nblk == 1) dec_gemv_kernel<SPW, 1, 1, EPI, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else if (tn == 1 && nblk == 2 && SPW <= 8) dec_gemv_kernel<SPW <= 8 ? SPW : 2, 1, 2, EPI, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else if (tn == 2 && nblk == 1 && WIDE && LOGITS) dec_gemv_kernel<WIDE ? SPW : 2, 2, 1, WIDE ? EPI : DE_LOGITS, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else if (tn == 4 && nblk == 1 && WIDE && LOGITS) dec_gemv_kernel<WIDE ? SPW : 2, 4, 1, WIDE ? EPI : DE_LOGITS, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else if (tn == 2 && nblk == 2 && WIDE) dec_gemv_kernel<WIDE ? SPW : 2, 2, 2, EPI, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else if (tn == 4 && nblk == 2 && WIDE) dec_gemv_kernel<WIDE ? SPW : 2, 4, 2, EPI, LN><<<grid, th, lds, s>>>(GEMV_ARGS(p));
    else { wm_set_error("dec_gemv: no kernel for the planned shape (tn %d, nblk %d, spw %d)", tn, nblk, SPW); return WM_ERR_INVALID; }
    WM_HIP(hipGetLastError());
    return WM_OK;
}

template <int EPI, bool LN>
int launch_gemv(wm_ctx *ctx, const DecGemvDev &p, const DecGemvPlan &pl) {
    switch (pl.spw) {
        case 2: return launch_gemv_shape<2, EPI, LN>(ctx, p, pl);
        case 4: return launch_gemv_shape<4, EPI, LN>(ctx, p, pl);
        case 5: return launch_gemv_shape<5, EPI, LN>(ctx, p, pl);
        case 6: return launch_gemv_shape<6, EPI, LN>(ctx, p, pl);
        case 8: return launch_gemv_shape<8, EPI, LN>(ctx, p, pl);
        case 10: return launch_gemv_shape<10, EPI, LN>(ctx, p, pl);
        case 12: return launch_gemv_shape<12, EPI, LN>(ctx, p, pl);
        default: wm_set_error("dec_gemv: unsupported k-steps per wave %d", pl.spw); return WM_ERR_INVALID;
    }
}

// every (epilogue, LayerNorm) pair the GEMV is instantiated for, with its profiler label (label_k: the label when K > N)
const struct GemvEpi {
    int epi;
    bool ln;
    const char *label, *label_k;
    int (*launch)(wm_ctx *, const DecGemvDev &, const DecGemvPlan &);
} kGemvEpi[] = {
    {DE_QKV, true, "dec_gemv_ln_qkv", nullptr, launch_gemv<DE_QKV, true>},
    {DE_QKV_P, true, "dec_gemv_ln_qkv", nullptr, launch_gemv<DE_QKV_P, true>},
    {DE_Q, true, "dec_gemv_ln_q", nullptr, launch_gemv<DE_Q, true>},
    {DE_GELU, true, "dec_gemv_ln_fc1", nullptr, launch_gemv<DE_GELU, true>},
    {DE_LOGITS, true, "dec_gemv_ln_logits", nullptr, launch_gemv<DE_LOGITS, true>},
    {DE_LOGITS_X, true, "dec_gemv_ln_logits_x", nullptr, launch_gemv<DE_LOGITS_X, true>},
    {DE_LOGITS_XR, true, "dec_gemv_ln_logits_xr", nullptr, launch_gemv<DE_LOGITS_XR, true>},
    {DE_LOGITS_XB, true, "dec_gemv_ln_logits_xb", nullptr, launch_gemv<DE_LOGITS_XB, true>},
    {DE_RESID, false, "dec_gemv_attn_out", "dec_gemv_fc2", launch_gemv<DE_RESID, false>},
    {DE_Q, false, "dec_gemv_plain", nullptr, launch_gemv<DE_Q, false>},
};

}  // namespace

int wm_dec_gemv(wm_ctx *ctx, const DecGemvArgs &a) {
    const bool ln = a.c1 != nullptr;
    WM_REQUIRE(!ln || a.stats_in, WM_ERR_INVALID,
               "dec_gemv: LayerNorm mode needs the producer's K/16 partial statistics (K a multiple of 64, <= 1280)");
    WM_REQUIRE(a.a != nullptr && a.W != nullptr, WM_ERR_INVALID, "dec_gemv: null operand");
    WM_REQUIRE(a.epi != DE_QKV_P || (a.panel >= 1 && a.panel <= WM_MAX_TEACHER_PANEL && a.pos_ptr), WM_ERR_INVALID,
               "dec_gemv: DE_QKV_P needs a panel width of 1 .. %d and the device position", WM_MAX_TEACHER_PANEL);
    WM_REQUIRE(!de_is_x(a.epi) || (a.x.par && a.pos_ptr), WM_ERR_INVALID, "dec_gemv: DE_LOGITS_X needs its state and the device position");
    WM_REQUIRE(!de_has_rep(a.epi) || (a.rep.par && a.rep.seen && a.rep.ban && (long)a.rep.words * 32 >= a.N), WM_ERR_INVALID,
               "dec_gemv: DE_LOGITS_XR needs the repetition-rule state");
    WM_REQUIRE(a.epi != DE_LOGITS_XB || (a.sb.hit && a.sb.woff && a.sb.ltot && (long)a.sb.words * 32 >= a.N), WM_ERR_INVALID,
               "dec_gemv: DE_LOGITS_XB needs the sequence-bias state");
    const GemvEpi *e = nullptr;
    for (const GemvEpi &c : kGemvEpi)
        if (c.epi == a.epi && c.ln == ln) e = &c;
    WM_REQUIRE(e, WM_ERR_INVALID, "dec_gemv: unsupported (epilogue %d, LayerNorm %d) pair", a.epi, (int)ln);
    DecGemvShape sh;
    sh.epi = a.epi; sh.ln = ln; sh.B = a.B; sh.N = a.N; sh.K = a.K;
    sh.has_pf = a.pf_ptr != nullptr; sh.pf_rows = a.pf_rows; sh.pf_k = a.pf_k; sh.pf_head_major = a.pf_head_major;
    DecGemvPlan pl;
    WM_TRY(wm_plan_gemv(sh, ctx->n_cus, g_wm_tuning, &pl));
    DecGemvDev p;
    memset(&p, 0, sizeof(p));
    p.B = a.B; p.N = a.N; p.K = a.K;
    p.W = a.W; p.c1 = a.c1; p.c2 = a.c2; p.a = a.a;
    p.stats_in = a.stats_in; p.stats_parts = a.K / 16; p.stats_out = a.stats_out;
    p.mean_in = a.mean_in; p.mean_out = a.mean_out;
    p.stats_stride = 2L * (a.epi == DE_RESID ? a.N : a.K);  // [parts <= d/16][16][2] floats per block of 16 rows
    p.out_f32 = a.out_f32; p.out_bf16 = a.out_bf16;
    p.kcache = a.kcache; p.vcache = a.vcache; p.pos_ptr = a.pos_ptr; p.n_ctx = a.n_ctx; p.n_head = a.n_head;
    p.ldo = a.ldo; p.tilemax = a.argmax; p.arg_first = a.arg_first; p.arg_last = a.arg_last;
    p.mask = a.mask; p.mask_words = a.mask_words; p.mask_first_pos = a.mask_first_pos;
    p.ts = a.ts;
    p.x = a.x;
    p.rep = a.rep;
    p.panel = a.panel;
    p.sb = a.sb;
    p.n_tiles = pl.n_tiles; p.bgroups = pl.bgroups; p.n_tg = pl.n_tg; p.n_tg_pad = pl.n_tg_pad;
    if (pl.pf_tiles) {   // (no warm-up: the pointer stays null)
        p.pf_ptr = (const char *)a.pf_ptr;
        p.pf_tile_bytes = pl.pf_tile_bytes; p.pf_tiles = pl.pf_tiles; p.pf_head_major = pl.pf_head_major;
    }
    WmProfScope ps(&ctx->prof, e->label_k && a.K > a.N ? e->label_k : e->label, ctx->stream);
    return e->launch(ctx, p, pl);
}

int wm_ln_fold(wm_ctx *ctx, const bf16_t *W, const float *g, const float *beta, const float *bias, int N, int K,
               bf16_t *Wf, float *c1, float *c2) {
    const int npad = (N + 15) / 16 * 16;
    ln_fold_kernel<<<npad, 256, 0, ctx->stream>>>(W, g, beta, bias, N, K, Wf, c1, c2);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_dec_embed(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, const WmEmbedDev &e, const int *off) {
    WmProfScope ps(&ctx->prof, "dec_embed", ctx->stream);
    dec_embed_kernel<<<B, 256, 0, ctx->stream>>>(seq, pos_ptr, B, e.emb, e.pemb, e.d, e.x, e.xb, e.stats_out, e.mean_buf, off);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_dec_embed_panel(wm_ctx *ctx, const int *seq, int seq_stride, const int *pos_ptr, int pos_add, int C, int w, int n_ctx,
                       const WmEmbedDev &e, const int *off) {
    WM_REQUIRE(w >= 1 && w <= WM_MAX_TEACHER_PANEL && C >= 1 && C * w <= WM_DEC_MAXB && seq_stride >= C, WM_ERR_INVALID,
               "dec_embed_panel: %d windows x %d positions (stride %d)", C, w, seq_stride);
    WmProfScope ps(&ctx->prof, "dec_embed_panel", ctx->stream);
    if (off)   // a ragged group: the windows' offsets
        dec_embed_panel_off_kernel<<<C * w, 256, 0, ctx->stream>>>(seq, seq_stride, pos_ptr, pos_add, w, e.emb, e.pemb, e.d, n_ctx, e.x,
                                                                  e.xb, e.stats_out, e.mean_buf, off);
    else
        dec_embed_panel_kernel<<<C * w, 256, 0, ctx->stream>>>(seq, seq_stride, pos_ptr, pos_add, w, e.emb, e.pemb, e.d, n_ctx, e.x, e.xb,
                                                              e.stats_out, e.mean_buf);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_dec_pos_add(wm_ctx *ctx, int *pos_ptr, int add) {
    dec_pos_add_kernel<<<1, 1, 0, ctx->stream>>>(pos_ptr, add);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// The launch-shape rules are the pure functions of dec_launch.cpp; these two read the process's tuning state for them.
int wm_dec_attn_splits(int B, int H) { return wm_dec_attn_splits(B, H, g_wm_tuning); }
bool wm_dec_xattn_fq_applies(int B, int H, int K, bool short_lived) { return wm_dec_xattn_fq_applies(B, H, K, short_lived, g_wm_tuning); }

namespace {
// the integers of the arguments, for the plan functions
DecAttnShape attn_shape(const DecAttnArgs &t) {
    DecAttnShape s;
    memset(&s, 0, sizeof(s));
    s.B = t.B; s.C = t.C; s.N = t.N; s.H = t.H; s.T_stride = t.T_stride; s.n_keys = t.n_keys; s.nsplit = t.nsplit;
    s.has_pos = t.pos_ptr != nullptr; s.has_part = t.part != nullptr; s.has_off = t.off != nullptr; s.short_lived = t.short_lived;
    s.has_pf = t.pf.ptr != nullptr; s.pf_rows = t.pf.rows; s.pf_k = t.pf.k;
    return s;
}
int launch_combine(wm_ctx *ctx, const DecAttnArgs &t, const DecAttnPlan &pl);   // (defined behind its first caller: keeps the kernels' order in the code object)
}  // namespace

// The cross-attention.  (The debug hooks also run it over a self-shaped cache.)
int wm_dec_attention(wm_ctx *ctx, const DecAttnArgs &t) {
    DecAttnPlan pl;
    WM_TRY(wm_plan_attention(attn_shape(t), ctx->n_cus, g_wm_tuning, &pl));
    {
        WmProfScope ps(&ctx->prof, "dec_attn_cross", ctx->stream);
        const dim3 grid(pl.grid_x, pl.grid_y);
        if (pl.variant == DAV_STREAM) {
            // the LDS reservation that keeps the launch at ONE workgroup per CU (wm_plan_attention) must be allowed first
            const int lds_pad = g_wm_tuning.xattn_lds_pad;
            static std::atomic<int> pad_set[64];  // per device (wm_multi: one process, every GPU of the node): the size allowed so far
            if (lds_pad > pad_set[ctx->device & 63].load(std::memory_order_acquire)) {
                WM_HIP(hipFuncSetAttribute((const void *)dec_xrows_attn_kernel<8, 4, WM_XATTN_NT>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_pad));
                pad_set[ctx->device & 63].store(lds_pad, std::memory_order_release);
            }
            const AttnCold cold = {t.att, t.part, (const char *)t.pf.ptr, pl.tile_bytes};
            dec_xrows_attn_kernel<8, 4, WM_XATTN_NT><<<grid, pl.block, pl.lds, ctx->stream>>>(
                t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a, pl.w.b, pl.w.c, cold);
        } else {
            const AttnCold cold = {t.att, t.part, nullptr, 0};
            if (pl.variant == DAV_FLAT)
                dec_xrows_attn_kernel<8, 4, WM_XATTN_NT><<<grid, pl.block, 0, ctx->stream>>>(
                    t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a, pl.w.b, pl.w.c, cold);
            else if (pl.variant == DAV_FLAT_DEEP_C)
                dec_rows_attn_kernel<8, 4, false, true><<<grid, pl.block, 0, ctx->stream>>>(
                    t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a, pl.w.b, pl.w.c, cold);
            else
                dec_rows_attn_kernel<8, 4, WM_XATTN_NT, true><<<grid, pl.block, 0, ctx->stream>>>(
                    t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a, pl.w.b, pl.w.c, cold);
        }
        WM_HIP(hipGetLastError());
    }
    return pl.combine_grid ? launch_combine(ctx, t, pl) : WM_OK;
}

namespace {
int launch_combine(wm_ctx *ctx, const DecAttnArgs &t, const DecAttnPlan &pl) {
    WmProfScope ps(&ctx->prof, "dec_attn_combine", ctx->stream);
    dec_attn_combine_kernel<8><<<pl.combine_grid, 64, 0, ctx->stream>>>(t.part, t.H, t.H * 64, t.att);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
}  // namespace

// Cross-attention of a candidate group (dec_xcand_attn_kernel): C windows x N candidates, q / att rows c * N + s, K/V
// [C][H][T_stride][64].  part: [C * N][H][8][66] floats, needed below 256 (window, head) pairs (the flat deal).
int wm_dec_attention_cand(wm_ctx *ctx, const DecAttnArgs &t) {
    DecAttnPlan pl;
    WM_TRY(wm_plan_attention_cand(attn_shape(t), ctx->n_cus, g_wm_tuning, &pl));
    {
        WmProfScope ps(&ctx->prof, "dec_attn_cross_cand", ctx->stream);
        const char *pf = pl.warm_tiles ? (const char *)t.pf.ptr : nullptr;
        switch (t.N) {
#define WM_XCAND_CASE(n)                                                                                              \
    case n:                                                                                                           \
        dec_xcand_attn_kernel<n, WM_XATTN_NT><<<pl.grid_x, pl.block, 0, ctx->stream>>>(                               \
            t.q, t.kc, t.vc, t.live, t.att, t.part, pl.w.a, pl.w.b, pl.w.c, pf, pl.warm_tiles ? pl.tile_bytes : 0);   \
        break
            WM_XCAND_CASE(1); WM_XCAND_CASE(2); WM_XCAND_CASE(3); WM_XCAND_CASE(4);
            WM_XCAND_CASE(5); WM_XCAND_CASE(6); WM_XCAND_CASE(7); WM_XCAND_CASE(8);
#undef WM_XCAND_CASE
        }
        WM_HIP(hipGetLastError());
    }
    return pl.combine_grid ? launch_combine(ctx, t, pl) : WM_OK;
}

// Fused cross_attn_ln + query projection + cross-attention (dec_xattn_fq_kernel): the latency shape of 96 .. 256 pairs
// (wm_dec_xattn_fq_applies; else the caller runs the two separate launches: same results either way).
int wm_dec_xattn_fq(wm_ctx *ctx, const DecGemvArgs &qa, const DecAttnArgs &t) {
    WM_REQUIRE(qa.c1 && qa.stats_in && qa.N == qa.K && qa.K == t.H * 64, WM_ERR_INVALID, "xattn_fq: not a LayerNorm-folded d x d query projection");
    DecAttnShape sh = attn_shape(t);
    sh.K = qa.K;
    DecAttnPlan pl;
    WM_TRY(wm_plan_xattn_fq(sh, ctx->n_cus, g_wm_tuning, &pl));
    WmProfScope ps(&ctx->prof, "dec_attn_cross_fq", ctx->stream);
    FqCold cold;
    cold.c1 = qa.c1; cold.c2 = qa.c2; cold.stats_in = qa.stats_in; cold.mean_in = qa.mean_in; cold.mean_out = qa.mean_out;
    cold.att = t.att; cold.stats_stride = 2L * qa.K; cold.K = qa.K; cold.N = qa.N;
    cold.n_wg = pl.n_wg;
    cold.pf_ptr = pl.warm_tiles ? (const char *)t.pf.ptr : nullptr;
    cold.pf_tile_bytes = pl.tile_bytes;
    const int grid = pl.grid_x;
    const size_t lds = (size_t)pl.lds;
    hipStream_t s = ctx->stream;
    switch (pl.spw) {
        case 2: dec_xattn_fq_kernel<2, WM_XATTN_NT><<<grid, 512, lds, s>>>(qa.W, qa.a, t.kc, t.vc, t.live, pl.w.a, pl.w.b, qa.K, cold); break;
        case 4: dec_xattn_fq_kernel<4, WM_XATTN_NT><<<grid, 512, lds, s>>>(qa.W, qa.a, t.kc, t.vc, t.live, pl.w.a, pl.w.b, qa.K, cold); break;
        case 5: dec_xattn_fq_kernel<5, WM_XATTN_NT><<<grid, 512, lds, s>>>(qa.W, qa.a, t.kc, t.vc, t.live, pl.w.a, pl.w.b, qa.K, cold); break;
        case 6: dec_xattn_fq_kernel<6, WM_XATTN_NT><<<grid, 512, lds, s>>>(qa.W, qa.a, t.kc, t.vc, t.live, pl.w.a, pl.w.b, qa.K, cold); break;
        default: wm_set_error("xattn_fq: unsupported k-steps per wave %d", pl.spw); return WM_ERR_INVALID;
    }
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_dec_self_attention(wm_ctx *ctx, const DecAttnArgs &t) {
    DecAttnPlan pl;
    WM_TRY(wm_plan_self_attention(attn_shape(t), ctx->n_cus, g_wm_tuning, &pl));
    WmProfScope ps(&ctx->prof, "dec_attn_self", ctx->stream);
    if (pl.variant == DAV_SELF_OFF) {
        const AttnColdOff cold_off = {t.off, t.att, nullptr, (const char *)t.pf.ptr, pl.tile_bytes};
        dec_rows_attn_kernel<4, 4, false, false, true><<<pl.grid_x, 256, 0, ctx->stream>>>(t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a,
                                                                                          pl.w.b, pl.w.c, cold_off);
    } else {
        const AttnCold cold = {t.att, nullptr, (const char *)t.pf.ptr, pl.tile_bytes};
        dec_rows_attn_kernel<4, 4, false><<<pl.grid_x, 256, 0, ctx->stream>>>(t.q, t.kc, t.vc, t.pos_ptr, t.live, pl.w.a, pl.w.b, pl.w.c, cold);
    }
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_dec_self_attention_panel(wm_ctx *ctx, const DecAttnArgs &t) {
    DecAttnPlan pl;
    WM_TRY(wm_plan_self_attention_panel(attn_shape(t), ctx->n_cus, g_wm_tuning, &pl));
    WmProfScope ps(&ctx->prof, "dec_attn_self", ctx->stream);
    if (pl.variant == DAV_SELF_OFF_PANEL) {   // a ragged group's prompt panel: t.off = the offsets of the step's C windows
        const AttnColdOffPanel cold_off = {t.off, t.N, t.att, nullptr, (const char *)t.pf.ptr, pl.tile_bytes};
        dec_rows_attn_kernel<4, 4, false, false, true, true><<<pl.grid_x, 256, 0, ctx->stream>>>(t.q, t.kc, t.vc, t.pos_ptr, nullptr, pl.w.a,
                                                                                                pl.w.b, pl.w.c, cold_off);
    } else {
        const AttnColdPanel cold = {t.N, t.att, nullptr, (const char *)t.pf.ptr, pl.tile_bytes};
        dec_rows_attn_kernel<4, 4, false, false, false, true><<<pl.grid_x, 256, 0, ctx->stream>>>(t.q, t.kc, t.vc, t.pos_ptr, nullptr, pl.w.a,
                                                                                                 pl.w.b, pl.w.c, cold);
    }
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_argmax_embed(wm_ctx *ctx, const unsigned long long *tilemax, int n_tiles, int B, int *seq, int *pos_ptr,
                    int n_prompt, int *result, int arg_first, int n_ctx, const WmEmbedDev &e, const WmTsDev &ts, int *arrive,
                    int fallback_tok, const WmStopDev &stop, const WmXDev &xd, const int *off) {
    WmProfScope ps(&ctx->prof, "argmax_embed", ctx->stream);
    // Rows per workgroup.  A row's 3 242 keys (26 KB) are what the kernel pulls, and ONE CU pulls ~25 GB/s: a workgroup per
    // row (all 16 waves on its keys, one trip) instead of a workgroup per 16 rows -- in situ at 56 rows 37.5 -> 23.2 us,
    // driver command +0.7 %, tiny.en x 8 -1.6 % per position (profiles/r05_latency_probe.txt, run Q).  With early stop on,
    // several workgroups cost two agent-scope fences for the live list, so a group of <= 16 rows stays on one workgroup there.
    int rpw = (arrive && (B > 16 || !stop.done)) ? 1 : 16;
    if (arrive && g_wm_tuning.argmax_rows_per_wg >= 1 && g_wm_tuning.argmax_rows_per_wg <= 16) rpw = g_wm_tuning.argmax_rows_per_wg;   // (probes)
    const int grid = arrive ? (B + rpw - 1) / rpw : 1;
    WM_REQUIRE(grid == 1 || B <= rpw * grid, WM_ERR_INVALID, "argmax_embed: bad grid");
    WM_REQUIRE(arrive || B <= 16, WM_ERR_INVALID, "argmax_embed: more than 16 rows need the arrival counter");
    if (xd.par) {
        WM_REQUIRE(pos_ptr != nullptr, WM_ERR_INVALID, "argmax_embed: the extended decode needs the device position");
        argmax_embed_x_kernel<<<grid, 1024, 0, ctx->stream>>>(tilemax, n_tiles, B, seq, pos_ptr, n_prompt, result, arg_first,
                                                              e.emb, e.pemb, e.d, n_ctx, e.x, e.xb, e.stats_out, ts, arrive,
                                                              fallback_tok, e.mean_buf, stop, rpw, xd, off);
    } else {
        argmax_embed_kernel<<<grid, 1024, 0, ctx->stream>>>(tilemax, n_tiles, B, seq, pos_ptr, n_prompt, result, arg_first,
                                                            e.emb, e.pemb, e.d, n_ctx, e.x, e.xb, e.stats_out, ts, arrive,
                                                            fallback_tok, e.mean_buf, stop, rpw, off);
    }
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_sample_noise(wm_ctx *ctx, uint64_t seed, int chunk, int gi, int n0, int count, float *out) {
    WM_REQUIRE(count >= 0 && n0 >= 0 && chunk >= 0 && gi >= 0 && out, WM_ERR_INVALID, "sample_noise: bad arguments");
    if (count == 0) return WM_OK;
    sample_noise_kernel<<<(count + 255) / 256, 256, 0, ctx->stream>>>((unsigned long long)seed, chunk, gi, n0, count, out);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_stop_init(wm_ctx *ctx, const WmStopDev &stop, int B) {
    dec_live_init_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(stop, B);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

namespace {
// state before the first sampled token: no text token may open the transcript (timestamps on), the first timestamp
// is at most max_initial; history empty
__global__ void ts_init_kernel(WmTsDev ts, int B) {
    const int b = threadIdx.x;
    if (b >= B) return;
    const int hi = ts.max_initial >= 0 && ts.ts_begin + ts.max_initial + 1 < ts.n_vocab ? ts.ts_begin + ts.max_initial + 1
                                                                                         : ts.n_vocab;
    *(int4 *)(ts.rng + b * 4) = make_int4(0, 0, ts.ts_begin, hi);
    *(int4 *)(ts.hist + b * 4) = make_int4(0, 0, 1, -1);
}
}  // namespace

int wm_ts_init(wm_ctx *ctx, const WmTsDev &ts, int B) {
    ts_init_kernel<<<1, WM_DEC_MAXB, 0, ctx->stream>>>(ts, B);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// softmax over logits[b][first .. first+n) -> probs[b][n] (openai-whisper detect_language: language-token probabilities)
namespace {
__global__ __launch_bounds__(128) void range_softmax_kernel(const float *__restrict__ logits, long ldo, int first, int n,
                                                            float *__restrict__ probs) {
    __shared__ float red[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *row = logits + (long)b * ldo + first;
    float m = -1e30f;
    for (int i = tid; i < n; i += 128) m = fmaxf(m, row[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(red[0], red[1]);
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < n; i += 128) s += __expf(row[i] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1]);
    for (int i = tid; i < n; i += 128) probs[(long)b * n + i] = __expf(row[i] - m) * inv;
}
}  // namespace

int wm_range_softmax(wm_ctx *ctx, const float *logits, long ldo, int B, int first, int n, float *probs) {
    range_softmax_kernel<<<B, 128, 0, ctx->stream>>>(logits, ldo, first, n, probs);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_fill_synthetic(wm_ctx *ctx, const WmTensor &t, uint32_t seed, int tensor_id, float gain) {
    if (t.kind == 4) return WM_OK;  // sinusoids are computed on the host (model.cpp)
    const unsigned key = [&] {
        unsigned x = seed + (unsigned)tensor_id * 0x9E3779B9u;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        return x;
    }();
    const double std = (t.kind == 0) ? 0.02 : 0.01;
    const float scale = (float)(std / 37837.22659);
    const int grid = (int)((t.n_elems + 255) / 256 < 16384 ? (t.n_elems + 255) / 256 : 16384);
    synth_fill_kernel<<<grid, 256, 0, ctx->stream>>>(t.ptr, t.is_bf16 ? 1 : 0, t.n_elems, key, scale, t.layout,
                                                     t.conv_c, t.conv_kpad, t.kind, gain);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// ------------------------------------------------------------------ launch-floor probe -----
namespace {
__global__ void trivial_kernel(int *p) {
    if (p && threadIdx.x == 0 && blockIdx.x == 0) *p = *p + 1;
}
}  // namespace
int wm_launch_trivial(wm_ctx *ctx, int *p, int grid) {
    trivial_kernel<<<grid, 64, 0, ctx->stream>>>(p);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

// ------------------------------------------------------------------ concurrency probe -------
namespace {
__global__ void spin_kernel(int *p, int cycles) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < cycles) __builtin_amdgcn_s_sleep(2);
    if (p && threadIdx.x == 0 && blockIdx.x == 0) *p = *p + 1;
}
}  // namespace
int wm_launch_spin(hipStream_t s, int *p, int grid, int cycles) {
    spin_kernel<<<grid, 256, 0, s>>>(p, cycles);
    return hipGetLastError() == hipSuccess ? WM_OK : WM_ERR_HIP;
}
