// Image sizing (crop -> resample -> window / zero pad -> mirror), the arithmetic shared by the gfx950 kernel
// (image_size.hip) and its host twin (host_image_size.cpp): Pillow's 8-bit ImagingResample restated.
//
// Per resampled axis (input length inS = the crop's, output length outS), all in double:
//     scale = inS / outS, fs = max(scale, 1), support = S * fs (S = 1 bilinear, 2 bicubic), ksize = (int)ceil(support) * 2 + 1
//     output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
//                      n = min((int)(center + support + 0.5), inS) - xmin,
//                      w[x] = filter((x + xmin - center + 0.5) * (1 / fs)), ww = sum in index order, p[x] = w[x] / ww
//     k[x] = (int)(p * 2^22 +- 0.5) (truncating cast), sample = clip((2^21 + sum pixel * k) >> 22, 0, 255) in int32
// An axis whose length does not change is not resampled: it is the identity row {xmin = xx, n = 1, k = 2^22}, which the
// sample formula returns unchanged, so both passes run the same code on every axis.
// Both users are compiled with -ffp-contract=off: a fused multiply-add in the filter polynomials or in p * 2^22 +- 0.5 would
// change coefficients by one unit and pixels with them.
#pragma once
#include <math.h>
#include <stdint.h>

#include "twin.hpp"

namespace wv {
namespace isz {

constexpr int kPrecisionBits = 22;
constexpr int kMaxDownscale = 64;
constexpr int kMaxKsize = 2 * (2 * kMaxDownscale) + 1;   // bicubic at 64x: support 128; what the limit on the scale protects

WV_HD double filter_value(int filter, double t)
{
    if (t < 0.0) t = -t;
    if (filter == WV_RESAMPLE_BILINEAR) return t < 1.0 ? 1.0 - t : 0.0;
    const double a = -0.5;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
}

// Taps a coefficient row of this axis can have: Pillow's ksize, but never more than the axis has samples (the bounds clamp
// at inS); 1 for an axis that is not resampled.
WV_HD int axis_ksize(int inS, int outS, int filter)
{
    if (inS == outS) return 1;
    double fs = (double)inS / (double)outS;
    if (fs < 1.0) fs = 1.0;
    const double support = (filter == WV_RESAMPLE_BILINEAR ? 1.0 : 2.0) * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    return ksize < inS ? ksize : inS;
}

// First source index and tap count of output index xx.  Both are non-decreasing in xx.
WV_HD void axis_bounds(int inS, int outS, int filter, int xx, int *xmin_out, int *n_out)
{
    if (inS == outS) {
        *xmin_out = xx;
        *n_out = 1;
        return;
    }
    const double scale = (double)inS / (double)outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == WV_RESAMPLE_BILINEAR ? 1.0 : 2.0) * fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inS) xmax = inS;
    *xmin_out = xmin;
    *n_out = xmax - xmin;
}

// The fixed-point coefficient row of output index xx into k[0 .. n); returns n, *xmin_out = first source index.
// The weights are evaluated twice (sum, then quotient) instead of being stored: the same values both times.
WV_HD int axis_coeffs(int inS, int outS, int filter, int xx, int32_t *k, int *xmin_out)
{
    int xmin, n;
    axis_bounds(inS, outS, filter, xx, &xmin, &n);
    *xmin_out = xmin;
    if (inS == outS) {
        k[0] = 1 << kPrecisionBits;
        return 1;
    }
    const double scale = (double)inS / (double)outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += filter_value(filter, (x + xmin - center + 0.5) * ss);
    for (int x = 0; x < n; ++x) {
        double p = filter_value(filter, (x + xmin - center + 0.5) * ss);
        if (ww != 0.0) p /= ww;
        const double scaled = p * (double)(1 << kPrecisionBits);
        k[x] = p < 0 ? (int)(-0.5 + scaled) : (int)(0.5 + scaled);
    }
    return n;
}

WV_HD int clip8(int32_t acc)
{
    const int v = acc >> kPrecisionBits;   // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- tile plan of the kernel --------------------------------------------------------------------------------------
// One workgroup owns tile_rows x tile_cols output pixels.  Its LDS holds the horizontally resampled source rows its output
// rows need (uint8, row pitch a multiple of 4) and the coefficient rows of its columns and rows.  The candidates form a
// chain in which every entry is no larger than the one before in both directions, and the LDS need grows with the tap
// counts: an image with fewer taps never gets a smaller tile than one with more, so the tile count of
// (max_out_h, max_out_w, max_ksize) bounds the tile count of every image of the launch.
struct TilePlan {
    int rows, cols;
    int span_cap;   // source rows the intermediate can hold
};

WV_HD int pitch_of(int cols) { return (cols * 3 + 3) & ~3; }

// Source rows that `rows` consecutive output rows can need: (rows - 1) * scale + 2 * support + 1, with
// scale <= max(1, (ksize - 1) / 2) and 2 * support <= ksize - 1 (ksize = 2 * ceil(support) + 1), one spare.  A tap count
// clamped to the axis length (axis_ksize) keeps the bound: no span is longer than the axis, and ksize + 1 is.
WV_HD int span_bound(int rows, int ksize_v)
{
    const int sb = (ksize_v - 1) / 2 > 1 ? (ksize_v - 1) / 2 : 1;
    return (rows - 1) * sb + ksize_v + 1;
}

WV_HD size_t lds_need(int rows, int cols, int ksize_h, int ksize_v)
{
    return (size_t)span_bound(rows, ksize_v) * pitch_of(cols) + (size_t)cols * (ksize_h + 2) * 4 + (size_t)rows * (ksize_v + 2) * 4;
}

constexpr int kTileChain = 11;

// (16,256) (8,256) (8,128) (4,128) (4,64) (2,64) (2,32) (1,32) (1,16) (1,8) (1,4)
WV_HD void tile_candidate(int i, int *rows, int *cols)
{
    const int r = 16 >> ((i + 1) / 2);
    *rows = r > 1 ? r : 1;
    *cols = i < 8 ? 256 >> (i / 2) : 32 >> (i - 7);
}

// rows = 0: nothing fits (never for ksize <= kMaxKsize and lds_bytes >= kMinLds)
WV_HD TilePlan tile_plan(int ksize_h, int ksize_v, size_t lds_bytes)
{
    TilePlan p = {0, 0, 0};
    for (int i = 0; i < kTileChain; ++i) {
        int r, c;
        tile_candidate(i, &r, &c);
        if (lds_need(r, c, ksize_h, ksize_v) <= lds_bytes) {
            p.rows = r;
            p.cols = c;
            p.span_cap = span_bound(r, ksize_v);
            return p;
        }
    }
    return p;
}

constexpr size_t kMinLds = 16 * 1024;
constexpr size_t kMaxLds = 64 * 1024;   // two workgroups and more stay resident in the CU's 160 KiB

}  // namespace isz
}  // namespace wv
