// Shared host/device helpers for libwvhash (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "twin.hpp"

namespace wv {

// Value of a kernel-selection / tuning switch: always NULL in libwvhash.so (tune_release.cpp), the environment variable of
// that name in libwvhash_diag.so (tune_diag.cpp).
const char *tune(const char *name);

// Checks the launch itself (asynchronous execution errors surface at the caller's next sync).
#define WV_CHECK_LAUNCH(what)                                                        \
    do {                                                                             \
        hipError_t e_ = hipGetLastError();                                           \
        if (e_ != hipSuccess) WV_FAIL(WV_EHIP, "%s: %s", what, hipGetErrorString(e_)); \
    } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t align_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

// Raises a kernel's dynamic-LDS limit where it asks for more than the 64 KB every kernel may have.
inline int set_lds_attr(const void *fn, size_t bytes, const char *what)
{
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) WV_FAIL(WV_EHIP, "%s: hipFuncSetAttribute(%zu): %s", what, bytes, hipGetErrorString(e));
    }
    return WV_OK;
}

// prepared-database blob = [distance-kernel tile image][ranking-kernel images: rank.hpp]
size_t dist_prepared_bytes(int64_t N, int words);
int dist_prepare(const uint64_t *db, void *dbP, int64_t N, int words, hipStream_t st);

constexpr int kWave = 64;
constexpr int kMaxLdsBytes = 160 * 1024;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// A byte behind an empty asm, for code that packs clamped bytes with `lo | hi << 8`: hipcc fuses two adjacent clamps that are
// packed that way into one v_ashr_pk_u8_i32, takes the upper 16 bits of its result for zero and ORs the other two bytes onto
// it -- on gfx950 those bits keep what the register held before (seen in image_size.hip as stray bits in bytes 2 and 3 of
// every dword of rows with an even tap count).  Through the asm every byte is shifted, clamped and converted on its own.
__device__ __forceinline__ uint32_t own_byte(int v)
{
    asm volatile("" : "+v"(v));
    return (uint32_t)v;
}

// count of set bits of `mask` strictly below this lane
__device__ __forceinline__ int mbcnt(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// Wave64 inclusive scan on the DPP network (no LDS round trips): row_shr 1/2/4/8 inside each row of 16
// lanes, then row_bcast15 / row_bcast31 carry the row totals forward (the sequence LLVM's atomic
// optimizer emits for gfx9).  ~6 VALU instructions instead of 6 ds_bpermute round trips.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// sum over the wave, returned in every lane
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(v), 63);
}

// Exclusive scan over the bins of per-bin totals held 3 bins per lane of one wave (lane l: bins 3l .. 3l + 2; 192 >=
// the 130 bins of the Hamming ranking): base[b] = sum of the bins below b.  Returns the sum of the bins below the lane's first.
__device__ __forceinline__ uint32_t bin_scan3(const uint32_t (&t)[3], int nbins, uint32_t *base, int lane)
{
    const int b0 = 3 * lane;
    const uint32_t incl = wave_incl_scan_u32(t[0] + t[1] + t[2]);
    const uint32_t excl = incl - (t[0] + t[1] + t[2]);
    if (b0 < nbins) base[b0] = excl;
    if (b0 + 1 < nbins) base[b0 + 1] = excl + t[0];
    if (b0 + 2 < nbins) base[b0 + 2] = excl + t[0] + t[1];
    return excl;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// GELU(v) = 0.5 v (1 + erf(v / sqrt 2)) (nn.GELU() default, multi_dino_attention.py:1098).  erfc(|x|) by Abramowitz &
// Stegun 7.1.26 (absolute error <= 1.5e-7, i.e. fp32 rounding of an O(1) value), 1 + erf taken as erfc(|x|) on the
// negative side so that nothing cancels: 14 instructions against ~40 of the library erff.  -DWV_HF_EXACT_ERF restores
// erff.  Used by the one-launch front (head_front.hip) and the bf16 products (head_bf16.hip).
__device__ __forceinline__ float gelu_erf(float v)
{
#ifdef WV_HF_EXACT_ERF
    return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
#else
    const float x = fabsf(v) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));   // v_rcp_f32 (1 ulp); the IEEE division is 11 instructions
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float erfc_abs = p * t * __expf(-x * x);
    return 0.5f * v * (v >= 0.f ? 2.0f - erfc_abs : erfc_abs);
#endif
}

}  // namespace wv
