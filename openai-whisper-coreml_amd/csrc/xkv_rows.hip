// xkv_rows.hip -- window sets (wm_windows_encode / wm_transcribe_windows): the copy between a decode group's cross-attention
// K/V cache and the window-major store of a set, in both directions.
//
// A pure streaming copy: 2 * n_text_layer slabs of H * 1500 * 64 bf16 per window (large-v2: 64 x 3.84 MB = 246 MB read and
// 246 MB written per row), nothing reused, no LDS.  What bounds such a kernel is the bytes a CU keeps in flight towards
// HBM: every lane issues kVec 16-byte loads before its first store (kVec x 16 B x 256 lanes = 16 KiB per workgroup) and a
// CU holds several of these small workgroups (no LDS, ~24 VGPRs), i.e. well past the ~32 KiB per CU a streaming kernel
// needs.  Consecutive lanes touch consecutive 16-byte words: every wave instruction is one contiguous 1 KiB.
// All offsets are 64-bit: a 128-window large-v2 set spans 31 GB.
#include "model.h"

namespace {
constexpr int kThreads = 256, kVec = 4;
constexpr int kChunk = kThreads * kVec;   // 16-byte words per workgroup

// grid (ceil(slab16 / kChunk), n_rows * L2): workgroup (x, b * L2 + l2) copies words [x * kChunk, ...) of slab l2 of group row b
template <bool TO_STORE>
__global__ __launch_bounds__(kThreads) void xkv_rows_kernel(uint4 *__restrict__ group, uint4 *__restrict__ store,
                                                            const int *__restrict__ rows, int row0, int L2,
                                                            long long group_rows, long long slab16) {
    const int b = blockIdx.y / L2, l2 = blockIdx.y % L2;
    const long long r = rows ? (long long)rows[b] : (long long)row0 + b;
    uint4 *g = group + ((long long)l2 * group_rows + b) * slab16;
    uint4 *s = store + (r * L2 + l2) * slab16;
    const uint4 *src = TO_STORE ? g : s;
    uint4 *dst = TO_STORE ? s : g;
    const long long i0 = (long long)blockIdx.x * kChunk + threadIdx.x;
    uint4 v[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const long long i = i0 + (long long)k * kThreads;
        if (i < slab16) v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const long long i = i0 + (long long)k * kThreads;
        if (i < slab16) dst[i] = v[k];
    }
}
}  // namespace

int wm_xkv_rows(wm_ctx *ctx, bf16_t *group, long group_rows, bf16_t *store, const int *d_rows, int row0, int n_rows, int L2,
                long slab, bool to_store) {
    WM_REQUIRE(group && store && n_rows >= 1 && n_rows <= group_rows && L2 >= 1 && row0 >= 0 && slab >= 8 && slab % 8 == 0,
               WM_ERR_INVALID, "xkv_rows: bad shape (rows %d of %ld, %d slabs of %ld elements)", n_rows, group_rows, L2, slab);
    WM_REQUIRE(((uintptr_t)group | (uintptr_t)store) % 16 == 0, WM_ERR_INVALID, "xkv_rows: buffers must be 16-byte aligned");
    WM_REQUIRE((long long)n_rows * L2 <= 65535, WM_ERR_INVALID, "xkv_rows: %d rows x %d slabs exceed one launch", n_rows, L2);
    const long long slab16 = slab / 8;
    const dim3 grid((unsigned)((slab16 + kChunk - 1) / kChunk), (unsigned)(n_rows * L2));
    WmProfScope ps(&ctx->prof, "xkv_rows", ctx->stream);
    if (to_store)
        xkv_rows_kernel<true><<<grid, kThreads, 0, ctx->stream>>>((uint4 *)group, (uint4 *)store, d_rows, row0, L2, group_rows, slab16);
    else
        xkv_rows_kernel<false><<<grid, kThreads, 0, ctx->stream>>>((uint4 *)group, (uint4 *)store, d_rows, row0, L2, group_rows, slab16);
    WM_HIP(hipGetLastError());
    return WM_OK;
}
