// logmel_shared.h -- the device pieces of the log-mel front end that more than one translation unit states the same way
// (frontend.hip: the stage kernels; streams.hip: the live-stream carry and window kernels): the sample conversion of
// the input dtypes, the monotone encoding of a maximum, and the dynamic-range clamp + affine of one value.
#pragma once
#include "wm_internal.h"

template <typename T>
__device__ __forceinline__ T load_sample(const void *pcm, int dtype, size_t idx) {
    if (dtype == WM_I16) return (T)((const short *)pcm)[idx] * (T)(1.0 / 32768.0);
    if (dtype == WM_F32) return (T)((const float *)pcm)[idx];
    return (T)((const double *)pcm)[idx];
}

// Monotone encodings so an unsigned atomicMax orders floating-point values.
__device__ __forceinline__ unsigned long long enc_max(float v) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (unsigned long long)u;
}
__device__ __forceinline__ unsigned long long enc_max(double v) {
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ void dec_max(unsigned long long e, float *out) {
    unsigned u = (unsigned)e;
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    *out = __uint_as_float(u);
}
__device__ __forceinline__ void dec_max(unsigned long long e, double *out) {
    unsigned long long u = (e & 0x8000000000000000ull) ? (e & 0x7fffffffffffffffull) : ~e;
    *out = __longlong_as_double((long long)u);
}

// the dynamic-range clamp and affine of one value (every stage-2 layout, and a live stream's window)
template <typename T>
__device__ __forceinline__ T clamp_affine(T x, unsigned long long gm) {
    T g;
    dec_max(gm, &g);
    const T fl = g - (T)8.0;
    x = (x > fl) ? x : fl;         // x.max(gmax - 8.0)   lib.rs:96
    return (x + (T)4.0) / (T)4.0;  // (.. + 4.0) / 4.0
}
