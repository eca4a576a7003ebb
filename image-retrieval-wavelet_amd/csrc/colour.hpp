// Colour jitter (brightness / contrast / saturation in a per-image order), the arithmetic shared by the gfx950 kernel
// (colour.hip) and its host twin (host_colour.cpp): Pillow's ImageEnhance restated.
//
// Every enhancement is Image.blend(degenerate, image, factor): per byte, with f the factor as fp32, d the degenerate byte and
// x the image byte,
//     t = (float)d + f * (float)(x - d)        one fp32 multiply, one fp32 add, never a fused multiply-add
//     byte = (uint8)t, truncated, after clamping t to [0, 255]
// (Pillow clamps only for f outside [0, 1]; inside it t lies between d and x, so the clamp changes nothing there.)
//     brightness: d = 0        saturation: d = L of the pixel        contrast: d = m for every byte of the image
//     L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16                            Pillow's convert("L")
//     m = int(mean(L) + 0.5) over the image as it is when contrast runs = (2 S + n) / (2 n) in integers, S = sum of L
// (the true quotient S / n differs from x.5 by at least 1 / (2 n) >= 1.8e-9 at the largest image, far more than a double
// ulp, so the integer form equals Pillow's double computation).
// Both users are compiled with -ffp-contract=off, and blend8 switches contraction off for itself as well.
#pragma once
#include <stdint.h>

#include "twin.hpp"

namespace wv {
namespace col {

constexpr int kMaxOps = 3;

WV_HD int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

WV_HD int blend8(int d, int x, float f)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float prod = f * (float)(x - d);
    float t = (float)d + prod;
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (int)t;
}

WV_HD int mean_from_sum(uint64_t sum, uint64_t count) { return (int)((2 * sum + count) / (2 * count)); }

// n_ops of a descriptor as the loops use it: a value outside 0..3 (the check refuses it) never indexes past kind[] / factor[]
WV_HD int op_count(const wv_colour_ops &o) { return o.n_ops < 0 ? 0 : (o.n_ops > kMaxOps ? kMaxOps : o.n_ops); }

// index of the contrast operation in the chain, -1 when it has none
WV_HD int contrast_index(const wv_colour_ops &o)
{
    const int n = op_count(o);
    for (int i = 0; i < n; ++i)
        if (o.kind[i] == WV_COLOUR_CONTRAST) return i;
    return -1;
}

// operations [first, last) of the chain on one pixel; m = the contrast mean (unused when the range holds no contrast)
WV_HD void run_ops(const wv_colour_ops &o, int first, int last, int m, int *r, int *g, int *b)
{
    for (int i = first; i < last; ++i) {
        const float f = o.factor[i];
        int d0 = 0, d1 = 0, d2 = 0;
        if (o.kind[i] == WV_COLOUR_CONTRAST) {
            d0 = d1 = d2 = m;
        } else if (o.kind[i] == WV_COLOUR_SATURATION) {
            d0 = d1 = d2 = luma(*r, *g, *b);
        }
        *r = blend8(d0, *r, f);
        *g = blend8(d1, *g, f);
        *b = blend8(d2, *b, f);
    }
}

}  // namespace col
}  // namespace wv
