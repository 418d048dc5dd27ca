// dec_close.h -- device helpers shared by the kernels that CLOSE a decode position: the step-closing arg-max of the greedy /
// sampling decode (dec_kernels.hip argmax_embed_body) and the beam-search close (beam.hip): bf16 conversion, the packed
// (value, ~index) arg-max key and the (max, sum exp) merge.
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

}  // namespace
