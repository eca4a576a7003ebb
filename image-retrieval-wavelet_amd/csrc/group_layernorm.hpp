// Grouped LayerNorm (include/wvhash.h: wv_group_layernorm), the arithmetic shared by the gfx950 kernel (group_layernorm.hip)
// and its host twin (host_group_layernorm.cpp): x [N][T][E] -> out [N][T][E], sequence n normalised over E with the affine
// parameters of group n / ceil(N / G) -- torch.chunk(G, 0), one nn.LayerNorm per chunk, torch.cat, in one pass.
//
// One row (E values) belongs to 64 lanes.  V = vec_of(E) consecutive values form one access; access k of a row (values
// k V .. k V + V - 1) belongs to lane k % 64, so a lane walks the accesses lane, lane + 64, lane + 128, ... in ascending order:
//     s_lane   = sum of its values, added one by one in ascending order, starting from 0
//     s        = xor butterfly over the 64 lanes (distances 32, 16, 8, 4, 2, 1: v += v of lane ^ d); fp32 addition is
//                commutative, so every lane ends with the same bits
//     mean     = s / (float)E
//     q_lane   = fmaf(d, d, q_lane) over its values in the same order, d = x - mean;  q = the same butterfly
//     rstd     = 1 / sqrtf(q / (float)E + eps)
//     out      = ((x - mean) * rstd) * gamma + beta            two multiplies and one add, never contracted
// All of it in fp32; bf16 is widened on load (exact) and rounded to nearest even on store.  Both users are compiled with
// -ffp-contract=off, and the kernel with correctly rounded fp32 division and square root, as the host's are: the twin,
// which replays the 64 lanes and the butterfly in a loop, equals the kernel bit for bit.
// V depends on E alone (never on a pointer's alignment), so the order of the sums does too.
#pragma once
#include <math.h>
#include <stdint.h>

#include "twin.hpp"

namespace wv {
namespace gln {

constexpr int kLanes = 64;
constexpr int kRegE = 512;          // rows of up to this many values stay in registers between the passes

WV_HD int vec_of(int E) { return E % 4 == 0 ? 4 : 1; }

// torch.chunk(G, 0) of N sequences: sequences per group (the last group may be shorter, trailing groups may be empty)
WV_HD int64_t group_chunk(int64_t N, int G) { return (N + G - 1) / G; }

WV_HD float widen_bf16(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

WV_HD uint16_t round_bf16(float f)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);      // NaN stays NaN (quiet)
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

WV_HD float load_value(const float *p) { return *p; }
WV_HD float load_value(const uint16_t *p) { return widen_bf16(*p); }
WV_HD void store_value(float *p, float v) { *p = v; }
WV_HD void store_value(uint16_t *p, float v) { *p = round_bf16(v); }

// f(c) for the first value c of every access of `lane`, ascending
template <class F>
WV_HD void for_lane_accesses(int E, int V, int lane, F f)
{
    for (int c = lane * V; c < E; c += kLanes * V) f(c);
}

WV_HD float add_value(float s, float x) { return s + x; }
WV_HD float add_square(float q, float x, float mean)
{
    const float d = x - mean;
    return fmaf(d, d, q);
}
WV_HD float mean_of(float s, int E) { return s / (float)E; }
WV_HD float rstd_of(float q, int E, float eps) { return 1.0f / sqrtf(q / (float)E + eps); }
WV_HD float affine(float x, float mean, float rstd, float gamma, float beta)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float centred = x - mean;
    const float scaled = centred * rstd;
    const float prod = scaled * gamma;
    return prod + beta;
}

// the pointer part of the argument check (after wv_group_layernorm_check and the zero-row return); `what` names the caller
int check_pointers(const char *what, const void *x, const void *out, const float *gamma, const float *beta);

}  // namespace gln
}  // namespace wv
