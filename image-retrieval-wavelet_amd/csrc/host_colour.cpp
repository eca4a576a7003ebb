// Host twin of the colour jitter kernel (colour.hip) and the one argument check of both: HOST pointers, no HIP call, no
// thread, no global state -> safe in forked DataLoader workers.  The per-pixel chain is the function the kernel compiles too
// (colour.hpp): the two agree byte for byte, and both equal Pillow's ImageEnhance applied in the same order.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "colour.hpp"

namespace {

using namespace wv::col;
using wv::kMaxImageSide;

int check_image(const wv_colour_ops &o, int i)
{
    if (o.h < 1) WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: h = %d (must be >= 1)", i, o.h);
    if (o.w < 1) WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: w = %d (must be >= 1)", i, o.w);
    if (o.h > kMaxImageSide) WV_FAIL(WV_ENOTSUP, "wv_colour_jitter: image %d: h = %d (limit %d)", i, o.h, kMaxImageSide);
    if (o.w > kMaxImageSide) WV_FAIL(WV_ENOTSUP, "wv_colour_jitter: image %d: w = %d (limit %d)", i, o.w, kMaxImageSide);
    if ((int64_t)o.row_bytes < 3 * (int64_t)o.w)
        WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: row_bytes = %d is shorter than a row of w = %d pixels", i, o.row_bytes, o.w);
    if (o.offset < 0) WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: offset = %lld is negative", i, (long long)o.offset);
    if (o.n_ops < 0 || o.n_ops > kMaxOps) WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: n_ops = %d (0 .. %d)", i, o.n_ops, kMaxOps);
    for (int k = 0; k < o.n_ops; ++k) {
        if (o.kind[k] != WV_COLOUR_BRIGHTNESS && o.kind[k] != WV_COLOUR_CONTRAST && o.kind[k] != WV_COLOUR_SATURATION)
            WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: kind[%d] = %d (0 = brightness, 1 = contrast, 2 = saturation)", i, k, o.kind[k]);
        for (int j = 0; j < k; ++j)
            if (o.kind[j] == o.kind[k]) WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: kind[%d] = %d is listed twice (kind[%d])", i, k, o.kind[k], j);
        if (!isfinite(o.factor[k]) || o.factor[k] < 0.0f)
            WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: factor[%d] = %g (finite and >= 0)", i, k, (double)o.factor[k]);
    }
    return WV_OK;
}

inline int64_t image_end(const wv_colour_ops &o) { return o.offset + (int64_t)(o.h - 1) * o.row_bytes + 3 * (int64_t)o.w; }

void run_image(uint8_t *img, const wv_colour_ops &o)
{
    if (o.n_ops == 0) return;
    uint8_t *base = img + o.offset;
    const int cpos = contrast_index(o);
    int m = 0;
    if (cpos >= 0) {
        uint64_t sum = 0;
        for (int y = 0; y < o.h; ++y) {
            const uint8_t *p = base + (int64_t)y * o.row_bytes;
            uint32_t row = 0;                                    // <= 16384 * 255
            for (int x = 0; x < o.w; ++x) {
                int r = p[3 * x], g = p[3 * x + 1], b = p[3 * x + 2];
                run_ops(o, 0, cpos, 0, &r, &g, &b);
                row += (uint32_t)luma(r, g, b);
            }
            sum += row;
        }
        m = mean_from_sum(sum, (uint64_t)o.h * (uint64_t)o.w);
    }
    for (int y = 0; y < o.h; ++y) {
        uint8_t *p = base + (int64_t)y * o.row_bytes;
        for (int x = 0; x < o.w; ++x) {
            int r = p[3 * x], g = p[3 * x + 1], b = p[3 * x + 2];
            run_ops(o, 0, o.n_ops, m, &r, &g, &b);
            p[3 * x] = (uint8_t)r;
            p[3 * x + 1] = (uint8_t)g;
            p[3 * x + 2] = (uint8_t)b;
        }
    }
}

}  // namespace

extern "C" int wv_colour_jitter_check(const wv_colour_ops *ops, int n)
{
    if (n < 0) WV_FAIL(WV_EINVAL, "wv_colour_jitter: n = %d is negative", n);
    if (n == 0) return WV_OK;
    if (!ops) WV_FAIL(WV_EINVAL, "wv_colour_jitter: ops is NULL");
    for (int i = 0; i < n; ++i) {
        const int rc = check_image(ops[i], i);
        if (rc != WV_OK) return rc;
    }
    int a, b;                                                   // the n images must not overlap
    if (wv::ranges_overlap(n, [&](int i) { return ops[i].offset; }, [&](int i) { return image_end(ops[i]); }, &a, &b))
        WV_FAIL(WV_EINVAL, "wv_colour_jitter: image %d: offset = %lld lies inside image %d (ends at %lld)", b, (long long)ops[b].offset, a,
                (long long)image_end(ops[a]));
    return WV_OK;
}

extern "C" int wv_colour_jitter_cpu(uint8_t *img, const wv_colour_ops *ops, int n)
{
    const int rc = wv_colour_jitter_check(ops, n);
    if (rc != WV_OK) return rc;
    if (n == 0) return WV_OK;
    if (!img) WV_FAIL(WV_EINVAL, "wv_colour_jitter_cpu: img is NULL");
    for (int i = 0; i < n; ++i) run_image(img, ops[i]);
    return WV_OK;
}
