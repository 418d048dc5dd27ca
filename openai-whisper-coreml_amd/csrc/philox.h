// philox.h -- Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants) and the Gumbel noise of wm_transcribe's temperature sampling.  Host and device: the GPU kernels and the
// CPU restatement in tests/ (a host build of this header) run the same arithmetic.
//
// Sampling at temperature T draws token n with probability softmax(logits / T) by the Gumbel-max trick: the arg-max of
// score(n) = logit(n) / T + g(n), g(n) = -log(-log u(n)), u(n) uniform in (0, 1).  The uniform of token n at generated
// index gi of chunk c (the chunk's index within the call) under a 64-bit seed is word (n & 3) of
//     philox4x32_10(counter = {n >> 2, gi, c, s}, key = {seed & 0xffffffff, seed >> 32})
// with s the candidate index of a best-of-N call and 0 in every other call,
// mapped to u = ((x >> 9) * 2 + 1) * 2^-24: exact in f32, strictly inside (0, 1).  One Philox call serves four ids.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WM_PHILOX_FN __host__ __device__ static inline
#else
#define WM_PHILOX_FN static inline
#endif

struct wm_philox4 {
    uint32_t v[4];
};

WM_PHILOX_FN void wm_philox_mulhilo(uint32_t a, uint32_t b, uint32_t *hi, uint32_t *lo) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    *lo = (uint32_t)p;
}

// ten rounds; the key is bumped by the Weyl constants between rounds
WM_PHILOX_FN wm_philox4 wm_philox4x32_10(wm_philox4 c, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        uint32_t hi0, lo0, hi1, lo1;
        wm_philox_mulhilo(0xD2511F53u, c.v[0], &hi0, &lo0);
        wm_philox_mulhilo(0xCD9E8D57u, c.v[2], &hi1, &lo1);
        wm_philox4 o;
        o.v[0] = hi1 ^ c.v[1] ^ k0;
        o.v[1] = lo1;
        o.v[2] = hi0 ^ c.v[3] ^ k1;
        o.v[3] = lo0;
        c = o;
    }
    return c;
}

// word (n & 3) of a Philox output, by selects: a run-time index into the array would put it in scratch memory on the GPU
WM_PHILOX_FN uint32_t wm_philox_word(const wm_philox4 &r, uint32_t n) {
    const uint32_t lo = (n & 1u) ? r.v[1] : r.v[0], hi = (n & 1u) ? r.v[3] : r.v[2];
    return (n & 2u) ? hi : lo;
}

// the 32-bit draw of token n (word n & 3 of the call that serves ids 4 (n >> 2) .. + 3)
WM_PHILOX_FN uint32_t wm_sample_bits(uint64_t seed, uint32_t chunk, uint32_t gi, uint32_t n) {
    wm_philox4 c;
    c.v[0] = n >> 2; c.v[1] = gi; c.v[2] = chunk; c.v[3] = 0u;
    const wm_philox4 r = wm_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return wm_philox_word(r, n);
}

// the same draw for CANDIDATE `cand` of the chunk (wm_transcribe_mel_best_of): the fourth counter word, 0 everywhere else --
// wm_sample_bits_cand(seed, chunk, 0, gi, n) == wm_sample_bits(seed, chunk, gi, n)
WM_PHILOX_FN uint32_t wm_sample_bits_cand(uint64_t seed, uint32_t chunk, uint32_t cand, uint32_t gi, uint32_t n) {
    wm_philox4 c;
    c.v[0] = n >> 2; c.v[1] = gi; c.v[2] = chunk; c.v[3] = cand;
    const wm_philox4 r = wm_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return wm_philox_word(r, n);
}

// u = ((x >> 9) * 2 + 1) * 2^-24 in (0, 1): 2^23 odd multiples of 2^-24, all exact in f32
WM_PHILOX_FN float wm_uniform_from_bits(uint32_t x) {
    return (float)(((x >> 9) << 1) | 1u) * 5.9604644775390625e-08f;
}

// -log(u) as used by the Gumbel map.  For u close to 1 the argument e = 1 - u is exact (u is a multiple of 2^-24) and
// the series e + e^2/2 + e^3/3 + e^4/4 (truncation < e^5 / 5: below f32 resolution for e < 2^-6) keeps the relative
// precision a log near 1 would lose; elsewhere one fast log.
#if defined(__HIP_DEVICE_COMPILE__)
#define WM_PHILOX_LOGF __logf
#else
#define WM_PHILOX_LOGF logf
#endif
#include <math.h>
WM_PHILOX_FN float wm_neg_log_u(float u) {
    const float e = 1.0f - u;
    if (e < 0.015625f) return e * (1.0f + e * (0.5f + e * (0.33333334f + e * 0.25f)));
    return -WM_PHILOX_LOGF(u);
}

// g(n) = -log(-log u(n)): finite for every draw (-log u lies in [5.96e-8, 16.64])
WM_PHILOX_FN float wm_gumbel_from_bits(uint32_t x) { return -WM_PHILOX_LOGF(wm_neg_log_u(wm_uniform_from_bits(x))); }
