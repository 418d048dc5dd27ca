// enc_kernels.hip -- encoder-side kernels other than the GEMM (SURVEY.md section 2:
// K6 LayerNorm, K8 encoder flash attention, plus the mel re-layout feeding conv1).
#include <type_traits>

#include "model.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) float f32x8;

__device__ __forceinline__ bf16_t f2bf(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
    return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
}

// ------------------------------------------------------------------ LayerNorm ----------
// One wave64 per row, f32 statistics (eps 1e-5), two passes over registers.  HBM-bound:
// reads d*4 B, writes d*2 B (bf16 GEMM operand) and/or d*4 B.
template <int MAXP>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x,
                                                        const float *__restrict__ g,
                                                        const float *__restrict__ b, int rows, int d,
                                                        bf16_t *__restrict__ ob, float *__restrict__ of) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    // 16 bytes per lane per load (one 1 KiB request per wave-instruction), all MAXP loads of the row in flight at once
    const float4 *xr = (const float4 *)(x + (size_t)row * d);
    const int np = d >> 2;  // float4 quads per row (d % 4 == 0, checked by the launcher)
    float4 v[MAXP];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        const int idx = i * 64 + lane;
        v[i] = (idx < np) ? xr[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        const int idx = i * 64 + lane;
        if (idx < np) {
            const float a = v[i].x - mean, c = v[i].y - mean, e = v[i].z - mean, f = v[i].w - mean;
            q += (a * a + c * c) + (e * e + f * f);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)d + 1e-5f);
    const float4 *g4 = (const float4 *)g, *b4 = (const float4 *)b;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        const int idx = i * 64 + lane;
        if (idx < np) {
            const float4 gg = g4[idx], bb = b4[idx];
            const float y0 = (v[i].x - mean) * rstd * gg.x + bb.x;
            const float y1 = (v[i].y - mean) * rstd * gg.y + bb.y;
            const float y2 = (v[i].z - mean) * rstd * gg.z + bb.z;
            const float y3 = (v[i].w - mean) * rstd * gg.w + bb.w;
            if (ob) ((uint2 *)(ob + (size_t)row * d))[idx] = make_uint2(pack2(y0, y1), pack2(y2, y3));
            if (of) ((float4 *)(of + (size_t)row * d))[idx] = make_float4(y0, y1, y2, y3);
        }
    }
}

// ------------------------------------------------------------------ mel re-layout -------
// mel f32 [B][C][3000] (the reference's encoder input layout, Whisper.swift:25) ->
// bf16 [B][3002][C] time-major with zero rows 0 and 3001 (zeroed once at allocation), so
// conv1's 3-tap window of frame t is the contiguous run mel_t[b][t .. t+2][:].
// WIN (wm_transcribe_mel): row b reads the window win[b] of a [C][T] block instead -- frames seek .. seek + n - 1, zeros
// from n to 3000 (openai-whisper pad_or_trim in mel space); the gather costs no pass of its own.
template <bool WIN>
__global__ __launch_bounds__(256) void mel_time_major_kernel(const float *__restrict__ mel, int C,
                                                             bf16_t *__restrict__ out, const WmMelWin *__restrict__ win) {
    __shared__ float tile[128][65];
    const int b = blockIdx.y, t0 = blockIdx.x * 64;
    size_t base = (size_t)b * C * WM_N_FRAMES;
    int T = WM_N_FRAMES, n = WM_N_FRAMES;
    if (WIN) {
        const WmMelWin w = win[b];
        base = (size_t)w.base + (size_t)w.seek;
        T = w.T;
        n = w.n;
    }
    for (int i = threadIdx.x; i < C * 64; i += 256) {
        const int c = i >> 6, t = i & 63;
        tile[c][t] = (t0 + t < n) ? mel[base + (size_t)c * T + t0 + t] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 64; i += 256) {
        const int t = i / C, c = i % C;
        if (t0 + t < WM_N_FRAMES) out[((size_t)b * 3002 + 1 + t0 + t) * C + c] = f2bf(tile[c][t]);
    }
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float *__restrict__ in,
                                                          bf16_t *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = f2bf(in[i]);
}

// ------------------------------------------------------------------ encoder attention ---
// Non-causal multi-head attention, head_dim 64, flash style (online softmax, fp32
// statistics, scores never leave registers).  One workgroup = 4 waves = 128 query rows of
// one (chunk, head); each wave owns 32 query rows.
//
// CDNA4-specific structure: the score tile is computed TRANSPOSED, S^T = K Q^T, with
// v_mfma_f32_32x32x16_bf16, so that lane l holds scores of ONE query (column l & 31):
// the softmax row reductions are in-register max3 chains plus a single exchange with lane
// l ^ 32 instead of butterfly shuffles.  P^T then feeds the second product directly as the
// B operand of O^T = V^T P^T (no transpose, no LDS round trip for P); V is stored
// transposed in HBM by the QKV GEMM epilogue so the A operand rows are contiguous, and the
// kv order inside a k-step is whatever order the accumulator registers hold (both operands
// use the same order, so the sum is unchanged).
//
// Round 4: the loop is bound by INSTRUCTION ISSUE, not by the matrix pipe (round 3: 16 MFMAs among ~200 instructions per
// wave and 64-key tile, ~8 issue slots per 32-cycle MFMA => MFMA-busy 0.40), so the per-score VALU work was cut to the
// two instructions that cannot go away (v_exp_f32, v_cvt_pk_bf16_f32):
//   * the query arrives PRE-SCALED by hd^-1/2 log2(e) (one multiply in the QKV GEMM epilogue, before its single bf16
//     rounding), and the running reference r of the online softmax enters the score product as the MFMA's C operand
//     (a separate 16-register tuple holding -r): the accumulator comes out as s - r in log2 units, p = exp2(acc);
//   * r is a LAGGED maximum: it moves (and O, l are rescaled, and the C tuple rewritten) only when a score of the tile
//     exceeds it by more than 2^8 -- on the first tile, and rarely afterwards; p <= 256 is exact enough in bf16 / f32;
//   * (measured, not adopted: the row sum l as a fifth accumulator fed by the same bf16 P^T fragments against an all-ones
//     A operand -- 4 MFMAs per tile instead of 16 packed adds; SUM_MFMA, debug knob enc_attn_mfma_sum.)
constexpr float ATT_RESCALE_THR = 8.0f;   // log2 units: p <= 2^8 before the reference moves

// K / V^T tiles in LDS (round 4, second half): a tile is 64 rows x 128 bytes (K: 64 keys x 64 dims; V^T: 64 dims x 64
// keys) = 8 KiB, brought in by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, no VGPR round trip, no ds_write) into
// a ring of three {K, V^T} slots: the tile after next is requested at the top of every tile and has a whole tile of
// compute to land (round 3 staged through registers and waited for its own loads at the end of the same tile: the lab
// -- tools/enc_attn_lab.hip -- attributed 28 % of the kernel to that).  LDS-DMA writes a wave's 64 x 16 bytes lane-
// linearly, so rows cannot be padded; bank conflicts are avoided by an XOR swizzle instead: rows are paired into 256-byte
// super-rows (16 chunks of 16 bytes), chunk p of super-row sr lives at position p ^ (sr & 15).  The swizzle is applied to
// the SOURCE address of each lane's DMA and again to the ds_read_b128 address (same involution) -- conflict-free for the
// fragment reads (lane = row % 32, half = lane / 32 reads chunk 2 i + half).  Both operands are read with ds_read_b128:
// V^T is stored in HBM with the two middle 4-key groups of every 16 keys swapped (att_vt_pos, written so by the QKV
// epilogue), which makes the 8 keys a lane multiplies in one MFMA k-step -- {0-3, 8-11} or {4-7, 12-15} of the 16, the
// order the score accumulators hold -- one contiguous 16-byte chunk.
constexpr int ATT_TILE_BYTES = 64 * 128;             // one operand tile
constexpr int ATT_SLOT_BYTES = 2 * ATT_TILE_BYTES;   // K + V^T
constexpr int ATT_RING = 3;

#define ATT_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")

// (Round 6, measured and dropped: 64-query workgroups of TWO waves for a single chunk -- Whisper-small x 1 chunk = 144
// workgroups of four waves on 256 CUs -> 288 of two; each wave then issues four DMA pieces per operand and tile, the
// kernel needs more than 256 VGPRs' worth of live state and runs at one wave per SIMD: encoder 1.457 -> 1.599 ms.)
template <bool SUM_MFMA, int NW = 4>
__global__ __launch_bounds__(NW * 64, 2) void enc_attn_kernel(const bf16_t *__restrict__ qk,
                                                          const bf16_t *__restrict__ vt,
                                                          bf16_t *__restrict__ att, int H, int S,
                                                          int S_pad, int d, int n_q, int n_bh) {
    __shared__ __attribute__((aligned(1024))) char ring[ATT_RING * ATT_SLOT_BYTES];
    // XCD-aware workgroup map.  The n_q query blocks of one (chunk, head) pair all stream the same 384 KB of K / V^T;
    // dispatch places workgroup w on XCD w % 8 (observed, not guaranteed: a wrong guess only costs speed), and each XCD
    // has a private L2 -- so the pairs are dealt to the XCDs (pair % 8) and the n_q blocks of a pair are CONSECUTIVE
    // workgroups of that XCD: K / V^T is fetched from HBM once per pair instead of once per XCD that happens to hold one
    // of its query blocks (round 1, grid (n_q, pairs): 537 MB fetched per launch for 93 MB of Q + K + V^T).
    const int xcd = blockIdx.x & 7, j0 = blockIdx.x >> 3;
    const int bh = (j0 / n_q) * 8 + xcd, qblk = j0 % n_q;
    if (bh >= n_bh) return;  // workgroup-uniform (pair count padded to a multiple of 8)
    const int b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hf = lane >> 5;
    constexpr int PPW = 8 / NW;   // 1-KiB DMA pieces per operand, tile and wave
    const int q = qblk * (NW * 32) + wave * 32 + ql;
    const int qc = q < S ? q : S - 1;
    const long ld = 2L * d;

    // Q^T B-fragments (pre-scaled queries): lane (col q, k = hf*8 + 16*ks .. +8)
    bf16x8 qf[4];
    {
        const bf16_t *qp = qk + ((long)b * S + qc) * ld + h * 64 + hf * 8;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) qf[s4] = *(const bf16x8 *)(qp + 16 * s4);
    }

    // ---- DMA sources.  Wave w issues two 1-KiB pieces per operand and tile: piece i covers super-rows (2 w + i) * 4 .. + 3;
    // lane l lands at super-row sr = that + l / 16, position l % 16, and therefore fetches logical chunk p = (l % 16) ^
    // (sr & 15) of the super-row: tile row 2 sr + p / 8, 16-byte chunk p % 8.
    const char *kbase = (const char *)(qk + (long)b * S * ld + d + h * 64);
    const char *vbase = (const char *)(vt + (long)(b * H + h) * 64 * S_pad);
    unsigned ksrc[PPW], vsrc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int sr = (wave * PPW + i) * 4 + (lane >> 4);
        const int pl = (lane & 15) ^ (sr & 15);
        const int row = 2 * sr + (pl >> 3), chunk = pl & 7;
        ksrc[i] = (unsigned)(row * ld * 2 + chunk * 16);
        vsrc[i] = (unsigned)(row * S_pad * 2 + chunk * 16);
    }
    const unsigned kstep = (unsigned)(64 * ld * 2);   // bytes between consecutive 64-key tiles of K (V^T: 128)
    auto issue = [&](unsigned slot_off, unsigned kadv, unsigned vadv) {   // slot_off: byte offset of the ring slot
        char *dk = ring + slot_off + wave * (PPW * 1024);   // wave-uniform; the hardware adds lane * 16
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kbase + (ksrc[i] + kadv)),
                                             (__attribute__((address_space(3))) void *)(dk + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vbase + (vsrc[i] + vadv)),
                                             (__attribute__((address_space(3))) void *)(dk + ATT_TILE_BYTES + i * 1024), 16, 0, 0);
        }
    };

    // ---- fragment read addresses: row = blk * 32 + ql, chunk = 2 i + hf  ->  blk * 4096 + (ql / 2) * 256 + (x0 ^ (i << 5))
    // with x0 = ((((ql & 1) << 3) | hf) ^ ((ql >> 1) & 15)) << 4: four lane constants, the block and the operand are
    // immediates, the ring slot one add per tile.
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)ring;
    const unsigned x0 = (unsigned)(((((ql & 1) << 3) | hf) ^ ((ql >> 1) & 15)) << 4);
    unsigned fa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = lds0 + (unsigned)((ql >> 1) * 256) + (x0 ^ (unsigned)(i << 5));

    f32x16 oacc[2], lacc, cneg;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        oacc[0][r] = 0.f;
        oacc[1][r] = 0.f;
        lacc[r] = 0.f;
        cneg[r] = 0.f;
    }
    float ref = 0.f;      // the running reference r (log2 units) of this lane's query; -r lives in cneg
    float lsum_v = 0.f;   // !SUM_MFMA: the row sum of this lane's half of the keys, f32 VALU adds
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    const int ntiles = (S + 63) / 64;
    issue(0u, 0u, 0u);
    if (ntiles > 1) issue((unsigned)ATT_SLOT_BYTES, kstep, 128u);
    // the Q loads and tile 0 have landed once at most the 2 PPW pieces of tile 1 are outstanding (vmcnt counts in order)
    if (ntiles > 1) {
        if constexpr (NW == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    // One 64-key tile.  FIRST: the reference is taken from this tile's maximum (unconditionally: l >= 1 from then on);
    // LAST: keys >= S masked (the only tile that can hold any).
    // (round 6) The ring-slot byte offset of the current tile (so) and of the slot the DMA fills (io) are carried as
    // wave-uniform counters that cycle 0 -> 16 K -> 32 K -> 0 (one add + compare + select on the scalar unit each) instead
    // of two `% 3` sequences per tile, and the fragment addresses are fa[] + so: 4 VALU adds instead of 12 in a loop that
    // is bound by VALU issue (profiles/r06_pmc_encoder_stalls.txt: 8.5 VALU instructions per MFMA).
    unsigned so = 0u, io = 2u * ATT_SLOT_BYTES;
    auto tile = [&](int j, auto first_tag, auto last_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr bool LAST = decltype(last_tag)::value;
        if (j + 2 < ntiles) issue(io, (unsigned)(j + 2) * kstep, (unsigned)(j + 2) * 128u);
        const unsigned a0 = fa[0] + so, a1 = fa[1] + so, a2 = fa[2] + so, a3 = fa[3] + so;
        so = so == 2u * ATT_SLOT_BYTES ? 0u : so + ATT_SLOT_BYTES;
        io = io == 2u * ATT_SLOT_BYTES ? 0u : io + ATT_SLOT_BYTES;
        // ---- S^T - r = K Q^T + (-r) : two 32-kv blocks, the reference enters as the C operand -----------
        bf16x8 kf[2][4];
        ATT_DSR(kf[0][0], a0, 0); ATT_DSR(kf[0][1], a1, 0); ATT_DSR(kf[0][2], a2, 0); ATT_DSR(kf[0][3], a3, 0);
        ATT_DSR(kf[1][0], a0, 4096); ATT_DSR(kf[1][1], a1, 4096); ATT_DSR(kf[1][2], a2, 4096); ATT_DSR(kf[1][3], a3, 4096);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(kf[0][0]), "+v"(kf[0][1]), "+v"(kf[0][2]), "+v"(kf[0][3]), "+v"(kf[1][0]), "+v"(kf[1][1]),
                       "+v"(kf[1][2]), "+v"(kf[1][3])::"memory");
        f32x16 st[2];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)   // the two chains interleaved: no MFMA waits for the one just issued
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
                st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][s4], qf[s4], s4 == 0 ? cneg : st[kb], 0, 0, 0);
        // V^T fragments of the tile, requested now: they land under the softmax
        bf16x8 vf[2][4];   // [eb][kb * 2 + j2]
        ATT_DSR(vf[0][0], a0, ATT_TILE_BYTES); ATT_DSR(vf[0][1], a1, ATT_TILE_BYTES);
        ATT_DSR(vf[0][2], a2, ATT_TILE_BYTES); ATT_DSR(vf[0][3], a3, ATT_TILE_BYTES);
        ATT_DSR(vf[1][0], a0, ATT_TILE_BYTES + 4096); ATT_DSR(vf[1][1], a1, ATT_TILE_BYTES + 4096);
        ATT_DSR(vf[1][2], a2, ATT_TILE_BYTES + 4096); ATT_DSR(vf[1][3], a3, ATT_TILE_BYTES + 4096);
        if constexpr (LAST) {  // mask kv >= S
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = j * 64 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
                    if (kv >= S) st[kb][r] = -1e30f;
                }
        }
        // ---- lagged reference: does any score of the tile exceed r by more than 2^THR? ----------------
        float mloc = st[0][0];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, st[kb][r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        if (FIRST || __builtin_amdgcn_ballot_w64(mloc > ATT_RESCALE_THR) != 0ull) {  // wave-uniform; rare after the first tile
            const float delta = FIRST ? mloc : fmaxf(mloc, 0.f);   // the reference only moves up
            ref += delta;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[kb][r] -= delta;
            if (!FIRST) {   // (first tile: O and l are still zero)
                const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    oacc[0][r] *= alpha;
                    oacc[1][r] *= alpha;
                    if (SUM_MFMA) lacc[r] *= alpha;
                }
                if (!SUM_MFMA) lsum_v *= alpha;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) cneg[r] = -ref;
        }
        // ONE register tuple for the reference across the rare branch: without this the compiler keeps a second copy and
        // refreshes it with 8 v_mov_b64 on EVERY tile (round 6, read off the ISA)
        asm volatile("" : "+v"(cneg));
        // ---- P^T = exp2(S^T - r) -> bf16;  O^T += V^T P^T;  l += 1^T P^T -------------------------------
        bf16x8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2) {
                f32x8 p8;
#pragma unroll
                for (int i = 0; i < 8; ++i) p8[i] = __builtin_amdgcn_exp2f(st[kb][8 * j2 + i]);
                pf[kb][j2] = __builtin_convertvector(p8, bf16x8);  // 4 x v_cvt_pk_bf16_f32
                if (!SUM_MFMA) lsum_v += ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]));
            }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(vf[0][0]), "+v"(vf[0][1]), "+v"(vf[0][2]), "+v"(vf[0][3]), "+v"(vf[1][0]), "+v"(vf[1][1]),
                       "+v"(vf[1][2]), "+v"(vf[1][3])::"memory");
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2) {
#pragma unroll
                for (int eb = 0; eb < 2; ++eb)
                    oacc[eb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[eb][kb * 2 + j2], pf[kb][j2], oacc[eb], 0, 0, 0);
                if (SUM_MFMA) lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pf[kb][j2], lacc, 0, 0, 0);
            }
        // the NEXT tile must have landed (this wave's share: everything but the 4 pieces just issued), and every wave must
        // be done reading this slot before the tile after next overwrites it
        if (!LAST) {
            if (j + 2 < ntiles) {
                if constexpr (NW == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
        }
    };
    if (ntiles == 1) {
        tile(0, std::true_type{}, std::true_type{});
    } else {
        tile(0, std::true_type{}, std::false_type{});
        for (int j = 1; j < ntiles - 1; ++j) tile(j, std::false_type{}, std::false_type{});
        tile(ntiles - 1, std::false_type{}, std::true_type{});
    }
    // ---- finalize: O^T[e][q] / l -> att[b*S + q][h*64 + e] (every row of the ones-product holds the query's sum) -----
    if (q < S) {
        const float inv = 1.0f / (SUM_MFMA ? lacc[0] : lsum_v + __shfl_xor(lsum_v, 32));
        bf16_t *op = att + ((long)b * S + q) * d + h * 64;
#pragma unroll
        for (int eb = 0; eb < 2; ++eb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int e0 = eb * 32 + 8 * g + 4 * hf;
                const unsigned lo = pack2(oacc[eb][4 * g + 0] * inv, oacc[eb][4 * g + 1] * inv);
                const unsigned hi = pack2(oacc[eb][4 * g + 2] * inv, oacc[eb][4 * g + 3] * inv);
                *(uint2 *)(op + e0) = make_uint2(lo, hi);
            }
    }
}

}  // namespace

int wm_layernorm(wm_ctx *ctx, const float *x, const float *g, const float *b, int rows, int d,
                 bf16_t *out_bf16, float *out_f32) {
    WM_REQUIRE(d % 4 == 0 && d <= 1280, WM_ERR_INVALID, "layernorm: d=%d unsupported (a multiple of 4, <= 1280)", d);
    WmProfScope ps(&ctx->prof, "layernorm", ctx->stream);
    const int grid = (rows + 3) / 4;
    if (d <= 256)
        layernorm_kernel<1><<<grid, 256, 0, ctx->stream>>>(x, g, b, rows, d, out_bf16, out_f32);
    else if (d <= 768)
        layernorm_kernel<3><<<grid, 256, 0, ctx->stream>>>(x, g, b, rows, d, out_bf16, out_f32);
    else
        layernorm_kernel<5><<<grid, 256, 0, ctx->stream>>>(x, g, b, rows, d, out_bf16, out_f32);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_mel_to_time_major(wm_ctx *ctx, const float *mel, int B, int n_mels, bf16_t *mel_t, const WmMelWin *d_win) {
    WM_REQUIRE(n_mels <= 128, WM_ERR_INVALID, "n_mels > 128");
    WmProfScope ps(&ctx->prof, "mel_time_major", ctx->stream);
    dim3 grid((WM_N_FRAMES + 63) / 64, B);
    if (d_win)
        mel_time_major_kernel<true><<<grid, 256, 0, ctx->stream>>>(mel, n_mels, mel_t, d_win);
    else
        mel_time_major_kernel<false><<<grid, 256, 0, ctx->stream>>>(mel, n_mels, mel_t, nullptr);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_f32_to_bf16(wm_ctx *ctx, const float *in, bf16_t *out, size_t n) {
    const int grid = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    f32_to_bf16_kernel<<<grid, 256, 0, ctx->stream>>>(in, out, n);
    WM_HIP(hipGetLastError());
    return WM_OK;
}

int wm_enc_attention(wm_ctx *ctx, const bf16_t *qk, const bf16_t *vt, bf16_t *att, int B, int H,
                     int S, int S_pad, int d) {
    WM_REQUIRE(d == H * 64, WM_ERR_INVALID, "attention: head_dim must be 64 (d=%d, H=%d)", d, H);
    WM_REQUIRE(S_pad % 64 == 0 && S_pad >= S, WM_ERR_INVALID, "attention: bad S_pad");
    WmProfScope ps(&ctx->prof, "enc_attention", ctx->stream);
    const int n_q = (S + 127) / 128, n_bh = B * H;
    const int grid = (n_bh + 7) / 8 * 8 * n_q;
    // row sums as f32 VALU adds; the ones-operand MFMA variant (4 more MFMAs, 16 fewer packed adds per tile) measured
    // 132 vs 119 us per layer at 8 chunks inside the model and is kept behind the debug knob only
    if (g_wm_tuning.enc_attn_mfma_sum)
        enc_attn_kernel<true><<<grid, 256, 0, ctx->stream>>>(qk, vt, att, H, S, S_pad, d, n_q, n_bh);
    else
        enc_attn_kernel<false><<<grid, 256, 0, ctx->stream>>>(qk, vt, att, H, S, S_pad, d, n_q, n_bh);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
