// Host twin of wv_lift_images (lifting_batched.hip) and the one argument check of both: HOST pointers, no HIP call, no
// thread, no global state -> safe in forked DataLoader workers.  The conversion and the lifting chain are the functions the
// kernel compiles too (lifting.hpp): the two agree bit for bit, and both equal the reference's float32 torch ops
// (ToTensor -> Normalize -> CustomTransform).  Plane by plane, level by level, through two scratch planes.
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

#include "lifting.hpp"

namespace {

using namespace wv::lift;
using wv::kMaxImageSide;

// one level of one plane: cur [h][w] (zero beyond, up to the padded size) -> ll, lh, hl, hh [nh][nw]; a NULL band is not formed
template <int BASIS>
void level_plane(const float *cur, int h, int w, const Consts &c, std::vector<float> &tmp, float *ll, float *lh, float *hl, float *hh)
{
    const int hp = padded(h, BASIS), wp = padded(w, BASIS), nh = hp / 2, nw = wp / 2;
    tmp.resize((size_t)hp * wp);               // rows [0, nh) = s, [nh, hp) = d
    for (int i = 0; i < nh; ++i)
        for (int x = 0; x < wp; ++x) {
            auto at = [&](int y) { return (y < h && x < w) ? cur[(size_t)y * w + x] : 0.0f; };
            float s, d;
            pair<BASIS>([&](int j) { return at(2 * j); }, [&](int j) { return at(2 * j + 1); }, nh, i, c, s, d);
            tmp[(size_t)i * wp + x] = s;
            tmp[(size_t)(nh + i) * wp + x] = d;
        }
    for (int y = 0; y < hp; ++y) {
        const float *row = tmp.data() + (size_t)y * wp;
        const bool srow = y < nh;
        float *ps = srow ? ll : lh, *pd = srow ? hl : hh;
        if (!ps && !pd) continue;
        const size_t o = (size_t)(srow ? y : y - nh) * nw;
        for (int i = 0; i < nw; ++i) {
            float s, d;
            pair<BASIS>([&](int j) { return row[2 * j]; }, [&](int j) { return row[2 * j + 1]; }, nw, i, c, s, d);
            if (srow) {
                ll[o + i] = s * c.sc_ll;
                if (hl) hl[o + i] = d;
            } else {
                lh[o + i] = s;
                hh[o + i] = d * c.sc_hh;
            }
        }
    }
}

}  // namespace

namespace wv {
namespace lift {

int convert_args(const char *who, int in_dtype, int C, int to_tensor, const float *mean, const float *std, Convert *cv)
{
    if (to_tensor != 0 && to_tensor != 1) WV_FAIL(WV_EINVAL, "%s: to_tensor = %d (0 or 1)", who, to_tensor);
    if ((mean == nullptr) != (std == nullptr)) WV_FAIL(WV_EINVAL, "%s: mean and std come together (both NULL = no Normalize)", who);
    if (to_tensor && in_dtype != WV_DT_U8) WV_FAIL(WV_EINVAL, "%s: to_tensor = 1 scales 8-bit images, in_dtype = %d is not WV_DT_U8", who, in_dtype);
    if (mean && in_dtype != WV_DT_U8)
        WV_FAIL(WV_ENOTSUP, "%s: Normalize is folded into the 8-bit conversion table only; normalise float32 input before the call", who);
    memset(cv, 0, sizeof(*cv));
    cv->to_tensor = to_tensor;
    cv->norm = mean != nullptr;
    for (int c = 0; mean && c < C && c < kMaxChannels; ++c) {
        if (!(mean[c] == mean[c]) || !(std[c] == std[c])) WV_FAIL(WV_EINVAL, "%s: mean[%d] / std[%d] is NaN", who, c, c);
        if (std[c] == 0.0f) WV_FAIL(WV_EINVAL, "%s: std[%d] = 0 leads to division by zero", who, c);
        cv->mean[c] = mean[c];
        cv->std[c] = std[c];
    }
    return WV_OK;
}

}  // namespace lift
}  // namespace wv

extern "C" int wv_lift_out_size(int n, int basis, int levels)
{
    if (n < 1 || (basis != kHaar && basis != kCdf97) || levels < 0 || levels > kMaxLevels) return 0;
    return out_size(n, basis, levels);
}

extern "C" int wv_lift_images_tile(int axis) { return axis == 0 ? 2 * kTilePairsH : (axis == 1 ? 2 * kTilePairsW : 0); }

extern "C" int wv_lift_images_check(int in_dtype, int in_layout, int B, int C, int H, int W, int basis, int levels, int ll_only)
{
    if (in_dtype != WV_DT_U8 && in_dtype != WV_DT_F32) WV_FAIL(WV_EINVAL, "wv_lift_images: in_dtype = %d (WV_DT_U8 or WV_DT_F32)", in_dtype);
    if (in_layout != WV_LAYOUT_NCHW && in_layout != WV_LAYOUT_NHWC)
        WV_FAIL(WV_EINVAL, "wv_lift_images: in_layout = %d (WV_LAYOUT_NCHW or WV_LAYOUT_NHWC)", in_layout);
    if (B < 0) WV_FAIL(WV_EINVAL, "wv_lift_images: B = %d is negative", B);
    if (C < 1) WV_FAIL(WV_EINVAL, "wv_lift_images: C = %d (must be >= 1)", C);
    if (H < 1) WV_FAIL(WV_EINVAL, "wv_lift_images: H = %d (must be >= 1)", H);
    if (W < 1) WV_FAIL(WV_EINVAL, "wv_lift_images: W = %d (must be >= 1)", W);
    if (basis != kHaar && basis != kCdf97) WV_FAIL(WV_EINVAL, "wv_lift_images: basis = %d (0 = haar, 1 = cdf97)", basis);
    if (levels < 0) WV_FAIL(WV_EINVAL, "wv_lift_images: levels = %d is negative", levels);
    if (ll_only != 0 && ll_only != 1) WV_FAIL(WV_EINVAL, "wv_lift_images: ll_only = %d (0 or 1)", ll_only);
    if (C > kMaxChannels) WV_FAIL(WV_ENOTSUP, "wv_lift_images: C = %d (limit %d)", C, kMaxChannels);
    if (H > kMaxImageSide) WV_FAIL(WV_ENOTSUP, "wv_lift_images: H = %d (limit %d)", H, kMaxImageSide);
    if (W > kMaxImageSide) WV_FAIL(WV_ENOTSUP, "wv_lift_images: W = %d (limit %d)", W, kMaxImageSide);
    if (levels > kMaxLevels) WV_FAIL(WV_ENOTSUP, "wv_lift_images: levels = %d (limit %d)", levels, kMaxLevels);
    if ((int64_t)B * C > INT32_MAX) WV_FAIL(WV_ENOTSUP, "wv_lift_images: B * C = %lld planes (limit 2^31 - 1)", (long long)B * C);
    return WV_OK;
}

extern "C" int wv_lift_images_cpu(const void *in, int in_dtype, int in_layout, int B, int C, int H, int W, int to_tensor, const float *mean,
                                  const float *std, int basis, int levels, int ll_only, float *out)
{
    int rc = wv_lift_images_check(in_dtype, in_layout, B, C, H, W, basis, levels, ll_only);
    if (rc != WV_OK) return rc;
    Convert cv;
    rc = convert_args("wv_lift_images_cpu", in_dtype, C, to_tensor, mean, std, &cv);
    if (rc != WV_OK) return rc;
    if (B == 0) return WV_OK;
    if (!in || !out) WV_FAIL(WV_EINVAL, "wv_lift_images_cpu: in / out is NULL");

    std::vector<float> table((size_t)256 * C);
    for (int c = 0; c < C; ++c)
        for (int x = 0; x < 256; ++x) table[(size_t)c * 256 + x] = convert_byte(cv, c, x);
    const Consts k = consts(basis);
    const int64_t sy = in_layout == WV_LAYOUT_NHWC ? (int64_t)W * C : W, sx = in_layout == WV_LAYOUT_NHWC ? C : 1;
    const int oh = out_size(H, basis, levels), ow = out_size(W, basis, levels);
    const int bands = levels == 0 || ll_only ? 1 : 4;
    std::vector<float> a((size_t)H * W), b, tmp;
    for (int64_t p = 0; p < (int64_t)B * C; ++p) {
        const int64_t img = p / C, c = p % C;
        const int64_t base = in_layout == WV_LAYOUT_NHWC ? img * H * W * C + c : p * H * W;
        float *dst = out + p * bands * oh * ow;
        a.resize((size_t)H * W);
        float *plane = levels == 0 ? dst : a.data();
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int64_t at = base + y * sy + x * sx;
                plane[(size_t)y * W + x] = in_dtype == WV_DT_U8 ? table[(size_t)c * 256 + static_cast<const uint8_t *>(in)[at]]
                                                                : static_cast<const float *>(in)[at];
            }
        std::vector<float> *cur = &a, *nxt = &b;
        int h = H, w = W;
        for (int l = 1; l <= levels; ++l) {
            const int nh = padded(h, basis) / 2, nw = padded(w, basis) / 2;
            const size_t band = (size_t)nh * nw;
            const bool last = l == levels;
            float *ll, *lh = nullptr, *hl = nullptr, *hh = nullptr;
            if (last) {
                ll = dst;
                if (!ll_only) lh = dst + band, hl = dst + 2 * band, hh = dst + 3 * band;
            } else {
                nxt->resize(band);
                ll = nxt->data();
            }
            if (basis == kHaar)
                level_plane<kHaar>(cur->data(), h, w, k, tmp, ll, lh, hl, hh);
            else
                level_plane<kCdf97>(cur->data(), h, w, k, tmp, ll, lh, hl, hh);
            std::swap(cur, nxt);
            h = nh, w = nw;
        }
    }
    return WV_OK;
}
