// dec_close.h -- device code shared by the kernels that CLOSE a decode position: the step-closing arg-max of the greedy /
// sampling decode (dec_kernels.hip argmax_embed_body), the beam-search close (beam.hip), the accept of a speculative
// round (spec.hip) and the close of a given-panel round (given_panel.hip).  First the small helpers (bf16 conversion, the packed (value, ~index) arg-max key and its butterfly
// maximum, the (max, sum exp) merge), then a row's close itself: the order-sensitive pieces whose bits make a beam of width 1
// the greedy decode and a speculative decode the plain one, each stated here and nowhere else.  An edit to one of them is an
// edit to all four closes (what holds them -- results, resources, time).  What the kernels BETWEEN the
// logits launch and a close share is in stored_row.h, what the two panel rounds share in panel_rows.h (section 10a).
#pragma once
#include "model.h"

namespace {

// f32 -> bf16 round-to-nearest-even: v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ bf16_t f2bf(float f) {
    const __bf16 h = (__bf16)f;
    return __builtin_bit_cast(bf16_t, h);
}
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float((unsigned)h << 16); }

__device__ __forceinline__ unsigned long long argmax_key(float v, int n) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)n);
}
// the value and the index of a non-zero key
__device__ __forceinline__ float argmax_key_value(unsigned long long key) {
    unsigned u = (unsigned)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int argmax_key_index(unsigned long long key) {
    return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}
// the maximum of a packed key over aligned groups of W lanes (a butterfly: every lane of a group gets it; any order, same bits)
template <int W>
__device__ __forceinline__ unsigned long long key_max_xor(unsigned long long key) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(key, o);
        key = ok > key ? ok : key;
    }
    return key;
}

// (max, sum exp) partials merged: commutative (no contraction), so a butterfly gives every lane the same bits
// (a plain two-float struct, selected field by field: HIP's float2 through selects and shuffles left the kernel a scratch copy)
struct Lse {
    float m, s;
};
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
    const float M = fmaxf(a.m, b.m);
    return Lse{M, __fadd_rn(__fmul_rn(a.s, __expf(a.m - M)), __fmul_rn(b.s, __expf(b.m - M)))};
}
__device__ __forceinline__ Lse lse_shfl_xor(Lse v, int o) { return Lse{__shfl_xor(v.m, o), __shfl_xor(v.s, o)}; }
__device__ __forceinline__ Lse lse_load(const float *p) {
    const float2 v = *(const float2 *)p;
    return Lse{v.x, v.y};
}

// ------------------------------------------------------------------ a row's close -------------------------------------
// The order-sensitive pieces of a row's close, stated ONCE: argmax_embed_body, the beam kernels, spec_accept_kernel and
// given_panel_close_kernel call these, which is what makes a beam of width 1 the greedy decode and a verified round the plain
// steps bit for bit (16 fixed tile segments, one wave per row for the merges, the decision and the embedding).  The callers
// keep their own guards (X, generated position, finished row, <|startoftranscript|> position, context end).

// One wave's share of a row's 16 FIXED tile segments of the WmXDev partials: segments pi, pi + P, ... of the row whose
// partials start at tile index rb; seg[sg] = allowed text (m, s), unfiltered (m, s) -- the latter merged when `sot` only.
// Each segment has one summation order whatever P is.
__device__ __forceinline__ void lse_row_segments(const WmXDev &xd, long rb, int n_tiles, bool sot, int pi, int P, int lane,
                                                 float (*seg)[4]) {
    const int cs = (n_tiles + 15) / 16;
    for (int sg = pi; sg < 16; sg += P) {
        const int lo = sg * cs, hi = lo + cs < n_tiles ? lo + cs : n_tiles;
        const Lse none{-1e30f, 0.f};
        Lse a = none, c = none;
        for (int t0 = lo + lane; t0 < hi; t0 += 64 * 4) {
            Lse va0 = none, va1 = none, va2 = none, va3 = none, vc0 = none, vc1 = none, vc2 = none, vc3 = none;
            if (t0 < hi) va0 = lse_load(xd.txt + (rb + t0) * 2);
            if (t0 + 64 < hi) va1 = lse_load(xd.txt + (rb + t0 + 64) * 2);
            if (t0 + 128 < hi) va2 = lse_load(xd.txt + (rb + t0 + 128) * 2);
            if (t0 + 192 < hi) va3 = lse_load(xd.txt + (rb + t0 + 192) * 2);
            if (sot) {   // wave-uniform
                if (t0 < hi) vc0 = lse_load(xd.all + (rb + t0) * 2);
                if (t0 + 64 < hi) vc1 = lse_load(xd.all + (rb + t0 + 64) * 2);
                if (t0 + 128 < hi) vc2 = lse_load(xd.all + (rb + t0 + 128) * 2);
                if (t0 + 192 < hi) vc3 = lse_load(xd.all + (rb + t0 + 192) * 2);
            }
            a = lse_merge(lse_merge(lse_merge(lse_merge(a, va0), va1), va2), va3);
            c = lse_merge(lse_merge(lse_merge(lse_merge(c, vc0), vc1), vc2), vc3);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a = lse_merge(a, lse_shfl_xor(a, o));
            c = lse_merge(c, lse_shfl_xor(c, o));
        }
        if (lane == 0) {
            seg[sg][0] = a.m; seg[sg][1] = a.s;
            seg[sg][2] = c.m; seg[sg][3] = c.s;
        }
    }
}

// The row's 16 segments merged in a fixed order (one wave): lt = allowed text, la = unfiltered; every lane gets both.
__device__ __forceinline__ void lse_row_total(const float (*seg)[4], int lane, Lse &lt, Lse &la) {
    if (lane < 16) {
        lt.m = seg[lane][0]; lt.s = seg[lane][1];
        la.m = seg[lane][2]; la.s = seg[lane][3];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        lt = lse_merge(lt, lse_shfl_xor(lt, o));
        la = lse_merge(la, lse_shfl_xor(la, o));
    }
    lt = Lse{__shfl(lt.m, 0), __shfl(lt.s, 0)};
    la = Lse{__shfl(la.m, 0), __shfl(la.s, 0)};
}

// Row b's timestamp tiles merged by one wave: the best allowed timestamp key and (M, S) = (max, sum exp(v - M)) over the
// allowed timestamps; every lane gets all three.
__device__ __forceinline__ void ts_row_merge(const WmTsDev &ts, int b, int n_tiles, int lane, unsigned long long &kts, float &M,
                                             float &S) {
    const int t_first = ts.ts_begin >> 4;
    kts = 0ull;
    M = -1e30f;
    for (int t = t_first + lane; t < n_tiles; t += 64) {
        const unsigned long long k2 = ts.key_ts[(long)b * n_tiles + t];
        kts = k2 > kts ? k2 : kts;
        M = fmaxf(M, ts.lse[((long)b * n_tiles + t) * 2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(kts, o);
        kts = ok > kts ? ok : kts;
        M = fmaxf(M, __shfl_xor(M, o));
    }
    S = 0.f;
    for (int t = t_first + lane; t < n_tiles; t += 64) {
        const float2 ms = *(const float2 *)(ts.lse + ((long)b * n_tiles + t) * 2);
        S += ms.y * __expf(ms.x - M);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
}

// The row's decision between its text and its timestamps, by one wave, every lane holding it.  key = the best allowed text
// key (0: none), text_max = the RAW maximum of the allowed text: the key's own value, or lt.m where the key may carry a
// perturbed score (the rule compares raw logits, as openai-whisper does).  ApplyTimestampRules: "if sum of probability over
// timestamps is above any other token, sample timestamp".
struct RowChoice {
    unsigned long long key;   // the winner; 0: nothing admissible (every allowed id suppressed, or NaN logits)
    bool forced;              // the sum rule forced a timestamp: the allowed set is the admissible timestamps alone
    Lse lts;                  // (max, sum exp) over the allowed timestamps
};
__device__ __forceinline__ RowChoice row_choose(const WmTsDev &ts, int b, int n_tiles, int lane, unsigned long long key, float text_max) {
    RowChoice c{key, false, Lse{-1e30f, 0.f}};
    if (ts.rng) {
        unsigned long long kts;
        float M, S;
        ts_row_merge(ts, b, n_tiles, lane, kts, M, S);
        const float text_best = key ? text_max : -1e30f;
        const float lse = S > 0.f ? M + __logf(S) : -1e30f;
        c.lts = Lse{M, S};
        c.forced = kts != 0ull && (key == 0ull || lse > text_best);
        if (c.forced) c.key = kts;                  // timestamps only
        else c.key = kts > key ? kts : key;         // arg-max over everything allowed
    }
    return c;
}
// log of the filtered distribution's normaliser (temperature 1): over the timestamps when one was forced, else over the
// allowed text and, under the rules, the timestamps
__device__ __forceinline__ float row_log_norm(const WmTsDev &ts, const RowChoice &c, Lse lt) {
    Lse al = lt;
    if (c.forced) al = c.lts;
    else if (ts.rng) al = lse_merge(lt, c.lts);
    return al.m + __logf(al.s);
}
// Where the winner value of id `tok` lies in WmXDev::win for the row whose partials start at tile index rb: [tile][text |
// timestamp].  The logits epilogue's layout, read by row_logprob and written by a hand-over (stored_row.h row_hand_over).
__device__ __forceinline__ long row_win_slot(const WmTsDev &ts, long rb, int tok) {
    const int side = (ts.rng && tok >= ts.ts_begin) ? 1 : 0;
    return (rb + (tok >> 4)) * 2 + side;
}
// log-prob of row b's winner under the filtered distribution; nothing admissible: -inf
__device__ __forceinline__ float row_logprob(const WmTsDev &ts, const WmXDev &xd, int b, int n_tiles, const RowChoice &c, Lse lt) {
    const float norm = row_log_norm(ts, c, lt);
    float lp = -INFINITY;
    if (c.key) lp = xd.win[row_win_slot(ts, (long)b * n_tiles, argmax_key_index(c.key))] - norm;
    return lp;
}
// no_speech_prob of row b from the unfiltered (max, sum exp)
__device__ __forceinline__ float row_no_speech(const WmXDev &xd, int b, Lse la) { return __expf(xd.ns_v[b] - la.m) / la.s; }

// The compact list of live rows the attention kernels walk, rebuilt by ONE wave from a per-row predicate (B <= WM_DEC_MAXB:
// two ballots): stop.live_rows and *stop.n_live.  is_live(b) is called exactly once per row b < B, by the row's lane.
template <class IsLive>
__device__ __forceinline__ void live_list_rebuild(const WmStopDev &stop, int B, int lane, IsLive is_live) {
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        const bool live = b < B && is_live(b < B ? b : 0);   // (the clamp: a load the compiler may issue ahead of the test)
        const unsigned long long m = __ballot(live);
        if (live) stop.live_rows[n + __popcll(m & ((1ull << lane) - 1ull))] = b;
        n += __popcll(m);
    }
    if (lane == 0) *stop.n_live = n;
}

// `tok` was sampled for a row whose timestamp-rule history is hs[4] (n_sampled, last_is_ts, prev_is_ts, last_ts): advance
// the history in place and return the ranges (text_lo, text_hi, ts_lo, ts_hi) of the next position.
__device__ __forceinline__ int4 ts_advance(const WmTsDev &ts, int *hs, int tok) {
    const int n_s = hs[0] + 1;
    const bool prev_ts = hs[0] < 1 || hs[1] != 0;  // penultimate_was_timestamp = len(seq) < 2 or seq[-2] >= begin
    const bool last_ts = tok >= ts.ts_begin;
    const int last_val = last_ts ? tok : hs[3];
    hs[0] = n_s; hs[2] = hs[1]; hs[1] = last_ts ? 1 : 0; hs[3] = last_val;
    int text_lo = 0, text_hi = ts.ts_begin, ts_lo = ts.ts_begin, ts_hi = ts.n_vocab;
    if (last_ts) {
        if (prev_ts) ts_hi = ts_lo;        // a pair was just closed: the next token is not a timestamp
        else text_lo = ts.eot;             // an opening timestamp needs its partner (or <|endoftext|>)
    }
    if (last_val >= 0) {                   // timestamps never decrease (and advance unless closing a pair)
        const int floor_ts = (last_ts && !prev_ts) ? last_val : last_val + 1;
        ts_lo = floor_ts > ts_lo ? floor_ts : ts_lo;
    }
    return make_int4(text_lo, text_hi, ts_lo, ts_hi);
}

// One wave embeds token `tok` at positional row `prow` into row b of the residual stream: x (f32), its mean-centred bf16
// copy xb (WL_TILED order), the row mean and the LayerNorm partial statistics the next layer-0 GEMV expects.
__device__ __forceinline__ void embed_row(long tok, int prow, int b, int lane, const bf16_t *__restrict__ emb,
                                          const float *__restrict__ pemb, int d, float *__restrict__ x, bf16_t *__restrict__ xb,
                                          float *__restrict__ stats_out, float *__restrict__ mean_buf) {
    float s1 = 0.f, s2 = 0.f;
    // the row stays in registers between the sums and the mean-centred bf16 copy (the first 512 columns: 8 values per lane; the
    // round-4 kernel re-read what it had just stored: a store -> load round trip through L2 on the step's tail)
    constexpr int EV = 8;   // (d <= 512 entirely: tiny, base -- where a step is 35 launches and this trip is 0.5 % of it)
    float ev[EV];
#pragma unroll
    for (int i = 0; i < EV; ++i) {
        const int j = lane + 64 * i;
        ev[i] = 0.f;
        if (j < d) {
            const float v = bf2f(emb[wm_tiled_offset((size_t)tok, (size_t)j, (size_t)d)]) + pemb[(long)prow * d + j];
            x[(long)b * d + j] = v;
            ev[i] = v;
            s1 += v;
            s2 += v * v;
        }
    }
    for (int j = lane + 64 * EV; j < d; j += 64) {  // (wider models than any Whisper: the re-reading path)
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
    {   // bf16 copy, mean-centred (see DecGemvDev::mean_in)
        const float mean = s1 / (float)d;
#pragma unroll
        for (int i = 0; i < EV; ++i) {
            const int j = lane + 64 * i;
            if (j < d) xb[wm_tiled_offset((size_t)b, (size_t)j, (size_t)d)] = f2bf(ev[i] - mean);
        }
        for (int j = lane + 64 * EV; j < d; j += 64)
            xb[wm_tiled_offset((size_t)b, (size_t)j, (size_t)d)] = f2bf(x[(long)b * d + j] - mean);
        if (lane == 0 && mean_buf) mean_buf[b] = mean;
    }
    if (stats_out) {  // one part (index 0) carries the row; the other d/16 - 1 parts the consumers sum are zero
        float *blk = stats_out + (long)(b >> 4) * (2 * d) + (b & 15) * 2;
        for (int pt = 1 + lane; pt < d / 16; pt += 64) *(float2 *)(blk + pt * 32) = make_float2(0.f, 0.f);
        if (lane == 0) *(float2 *)blk = make_float2(s1, s2);
    }
}

}  // namespace
