// Host twin of the image sizing kernel (image_size.hip) and the one argument check of both: HOST pointers, no HIP call, no
// thread, no global state -> safe in forked DataLoader workers.  The coefficient rows come from the routine the kernel
// compiles too (image_size.hpp), the rest is integer arithmetic: the two agree byte for byte, and both equal Pillow's
// Image.resize.  Only what the written window needs is computed: its columns, and the source rows its rows reach.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "image_size.hpp"

namespace {

using namespace wv::isz;
using wv::kMaxImageSide;

int check_stage(const wv_size_stage &s, int i)
{
#define IS_SIDE(f)                                                                                           \
    do {                                                                                                     \
        if (s.f < 1) WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: " #f " = %d (must be >= 1)", i, (int)s.f);  \
        if (s.f > kMaxImageSide)                                                                             \
            WV_FAIL(WV_ENOTSUP, "wv_image_size: stage %d: " #f " = %d (limit %d)", i, (int)s.f, kMaxImageSide); \
    } while (0)
    IS_SIDE(src_h);
    IS_SIDE(src_w);
    IS_SIDE(crop_h);
    IS_SIDE(crop_w);
    IS_SIDE(res_h);
    IS_SIDE(res_w);
    IS_SIDE(out_h);
    IS_SIDE(out_w);
#undef IS_SIDE
    if (s.crop_y < 0 || s.crop_y > s.src_h - s.crop_h)
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: crop_y = %d with crop_h = %d leaves src_h = %d", i, s.crop_y, s.crop_h, s.src_h);
    if (s.crop_x < 0 || s.crop_x > s.src_w - s.crop_w)
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: crop_x = %d with crop_w = %d leaves src_w = %d", i, s.crop_x, s.crop_w, s.src_w);
    if (s.filter != WV_RESAMPLE_BILINEAR && s.filter != WV_RESAMPLE_BICUBIC)
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: filter = %d (2 = bilinear, 3 = bicubic)", i, s.filter);
    if (s.flip != 0 && s.flip != 1) WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: flip = %d (0 or 1)", i, s.flip);
    if ((int64_t)s.src_row_bytes < 3 * (int64_t)s.src_w)
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: src_row_bytes = %d is shorter than a row of src_w = %d pixels", i, s.src_row_bytes, s.src_w);
    if ((int64_t)s.dst_row_bytes < 3 * (int64_t)s.out_w)
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: dst_row_bytes = %d is shorter than a row of out_w = %d pixels", i, s.dst_row_bytes, s.out_w);
    if (s.src_offset < 0) WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: src_offset = %lld is negative", i, (long long)s.src_offset);
    if (s.dst_offset < 0) WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: dst_offset = %lld is negative", i, (long long)s.dst_offset);
    if (s.win_y < -kMaxImageSide || s.win_y > kMaxImageSide)
        WV_FAIL(WV_ENOTSUP, "wv_image_size: stage %d: win_y = %d (limit +-%d)", i, s.win_y, kMaxImageSide);
    if (s.win_x < -kMaxImageSide || s.win_x > kMaxImageSide)
        WV_FAIL(WV_ENOTSUP, "wv_image_size: stage %d: win_x = %d (limit +-%d)", i, s.win_x, kMaxImageSide);
    // the limit on the scale bounds the taps of a coefficient row (kMaxKsize); an axis of no more samples than that is inside
    // it at any scale: its rows cannot have more taps than it has samples
    if ((int64_t)s.crop_h > (int64_t)kMaxDownscale * s.res_h && s.crop_h > kMaxKsize)
        WV_FAIL(WV_ENOTSUP, "wv_image_size: stage %d: crop_h = %d to res_h = %d is a down-scale above %d", i, s.crop_h, s.res_h, kMaxDownscale);
    if ((int64_t)s.crop_w > (int64_t)kMaxDownscale * s.res_w && s.crop_w > kMaxKsize)
        WV_FAIL(WV_ENOTSUP, "wv_image_size: stage %d: crop_w = %d to res_w = %d is a down-scale above %d", i, s.crop_w, s.res_w, kMaxDownscale);
    return WV_OK;
}

inline int64_t dst_end(const wv_size_stage &s) { return s.dst_offset + (int64_t)(s.out_h - 1) * s.dst_row_bytes + 3 * (int64_t)s.out_w; }

struct Axis {
    std::vector<int32_t> k;      // [count][ksize]
    std::vector<int> xmin, n;    // [count]
    int ksize = 1;
};

// coefficient rows of output indices [first, first + count)
void make_axis(Axis &a, int inS, int outS, int filter, int first, int count)
{
    a.ksize = axis_ksize(inS, outS, filter);
    a.k.assign((size_t)count * a.ksize, 0);
    a.xmin.resize(count);
    a.n.resize(count);
    for (int j = 0; j < count; ++j) a.n[j] = axis_coeffs(inS, outS, filter, first + j, &a.k[(size_t)j * a.ksize], &a.xmin[j]);
}

void run_stage(const uint8_t *src, uint8_t *dst, const wv_size_stage &s)
{
    const uint8_t *img = src + s.src_offset + (int64_t)s.crop_y * s.src_row_bytes + 3 * (int64_t)s.crop_x;
    uint8_t *out = dst + s.dst_offset;
    // rows / columns of the resampled image that the window shows
    const int ry0 = std::max(s.win_y, 0), ry1 = std::min(s.win_y + s.out_h, s.res_h);
    const int rx0 = std::max(s.win_x, 0), rx1 = std::min(s.win_x + s.out_w, s.res_w);
    for (int oy = 0; oy < s.out_h; ++oy) memset(out + (int64_t)oy * s.dst_row_bytes, 0, 3 * (size_t)s.out_w);
    if (ry1 <= ry0 || rx1 <= rx0) return;
    const int nrow = ry1 - ry0, ncol = rx1 - rx0;
    Axis ah, av;
    make_axis(ah, s.crop_w, s.res_w, s.filter, rx0, ncol);
    make_axis(av, s.crop_h, s.res_h, s.filter, ry0, nrow);
    const int srow0 = av.xmin[0], srow1 = av.xmin[nrow - 1] + av.n[nrow - 1];
    std::vector<uint8_t> mid((size_t)(srow1 - srow0) * ncol * 3);
    for (int r = srow0; r < srow1; ++r) {                       // horizontal pass: source row r -> ncol pixels
        const uint8_t *line = img + (int64_t)r * s.src_row_bytes;
        uint8_t *m = &mid[(size_t)(r - srow0) * ncol * 3];
        for (int c = 0; c < ncol; ++c) {
            const int32_t *k = &ah.k[(size_t)c * ah.ksize];
            const uint8_t *p = line + 3 * (size_t)ah.xmin[c];
            int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < ah.n[c]; ++x) {
                a0 += p[3 * x] * k[x];
                a1 += p[3 * x + 1] * k[x];
                a2 += p[3 * x + 2] * k[x];
            }
            m[3 * c] = (uint8_t)clip8(a0);
            m[3 * c + 1] = (uint8_t)clip8(a1);
            m[3 * c + 2] = (uint8_t)clip8(a2);
        }
    }
    for (int j = 0; j < nrow; ++j) {                            // vertical pass, window, mirror
        const int32_t *k = &av.k[(size_t)j * av.ksize];
        const uint8_t *m = &mid[(size_t)(av.xmin[j] - srow0) * ncol * 3];
        uint8_t *o = out + (int64_t)(ry0 + j - s.win_y) * s.dst_row_bytes;
        for (int c = 0; c < ncol; ++c) {
            const int wx = rx0 + c - s.win_x;                   // column inside the window
            const int ox = s.flip ? s.out_w - 1 - wx : wx;
            for (int ch = 0; ch < 3; ++ch) {
                int32_t a = 1 << (kPrecisionBits - 1);
                for (int y = 0; y < av.n[j]; ++y) a += m[((size_t)y * ncol + c) * 3 + ch] * k[y];
                o[3 * (size_t)ox + ch] = (uint8_t)clip8(a);
            }
        }
    }
}

}  // namespace

extern "C" int wv_image_size_check(const wv_size_stage *stages, int n)
{
    if (n < 0) WV_FAIL(WV_EINVAL, "wv_image_size: n = %d is negative", n);
    if (n == 0) return WV_OK;
    if (!stages) WV_FAIL(WV_EINVAL, "wv_image_size: stages is NULL");
    for (int i = 0; i < n; ++i) {
        const int rc = check_stage(stages[i], i);
        if (rc != WV_OK) return rc;
    }
    int a, b;                                                   // the destinations of the n images must not overlap
    if (wv::ranges_overlap(n, [&](int i) { return stages[i].dst_offset; }, [&](int i) { return dst_end(stages[i]); }, &a, &b))
        WV_FAIL(WV_EINVAL, "wv_image_size: stage %d: dst_offset = %lld lies inside the destination of stage %d (ends at %lld)", b,
                (long long)stages[b].dst_offset, a, (long long)dst_end(stages[a]));
    return WV_OK;
}

extern "C" int wv_image_size_cpu(const uint8_t *src, uint8_t *dst, const wv_size_stage *stages, int n)
{
    const int rc = wv_image_size_check(stages, n);
    if (rc != WV_OK) return rc;
    if (n == 0) return WV_OK;
    if (!src || !dst) WV_FAIL(WV_EINVAL, "wv_image_size_cpu: src / dst is NULL");
    for (int i = 0; i < n; ++i) run_stage(src, dst, stages[i]);
    return WV_OK;
}
