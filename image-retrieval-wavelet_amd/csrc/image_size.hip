// Image sizing on the GPU: crop -> resample -> window / zero pad -> mirror for a ragged batch of 3-channel uint8 HWC images,
// one launch per stage (include/wvhash.h: wv_image_size).  Pillow's 8-bit resampler restated (image_size.hpp) -- the
// coefficient rows come from the routine the host twin compiles too, everything after them is int32 arithmetic.
//
// Grid = (output tiles, images), 256 threads.  A workgroup owns tile_rows x tile_cols output pixels of one image:
//   1. it reads its descriptor and picks the image's tile from the image's own tap counts (isz::tile_plan);
//   2. one thread per coefficient row: the rows of its output columns and output rows go to LDS (fp64, a few taps each);
//   3. the source-row span [first row's ymin, last row's ymin + n) follows from the vertical bounds; the horizontal pass
//      runs for exactly those rows and the tile's columns from global memory into LDS as uint8 -- the rounded
//      intermediate.  It is stored in OUTPUT column order (mirrored when flip is set, zero where the window hangs over
//      the resampled image), so that the vertical pass is a plain weighted sum of byte rows;
//   4. barrier; the vertical pass takes four consecutive output bytes per thread from dword LDS reads and writes them with
//      one dword store when the destination row is 4-byte aligned (byte stores otherwise and at the row's end).
// Neighbouring tiles and neighbouring output columns re-read source bytes; those hit the vector L1 / L2.
// Everything a thread writes lies inside its image's out_h x out_w rows at dst_offset: the tile is clipped to them first.
#include "common.hpp"
#include "image_size.hpp"

namespace wv {
namespace {

using namespace isz;

constexpr int kThreads = 256;

// clip8 as a byte of its own (common.hpp: own_byte), safe to pack with its neighbours
__device__ __forceinline__ uint32_t clip8_byte(int32_t acc) { return own_byte(clip8(acc)); }

__device__ __forceinline__ int ceil_log2(int v) { return v > 1 ? 32 - __builtin_clz((unsigned)(v - 1)) : 0; }

__global__ __launch_bounds__(kThreads) void image_size_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                              const wv_size_stage *__restrict__ stages, int lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const wv_size_stage s = stages[blockIdx.y];
    const int ksz_h = axis_ksize(s.crop_w, s.res_w, s.filter), ksz_v = axis_ksize(s.crop_h, s.res_h, s.filter);
    const TilePlan plan = tile_plan(ksz_h, ksz_v, (size_t)lds_bytes);
    if (plan.rows == 0) return;
    const int tiles_x = (s.out_w + plan.cols - 1) / plan.cols, tiles_y = (s.out_h + plan.rows - 1) / plan.rows;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int oy0 = ty * plan.rows, ox0 = tx * plan.cols;
    const int nrows = min(plan.rows, s.out_h - oy0), ncols = min(plan.cols, s.out_w - ox0);
    const int pitch = pitch_of(ncols), row_bytes = ncols * 3;

    // LDS: [intermediate span_cap x pitch][kh: cols x ksz_h][hmin, hn: cols][kv: rows x ksz_v][vmin, vn: rows]
    uint8_t *mid = lds;
    int32_t *kh = reinterpret_cast<int32_t *>(lds + (size_t)plan.span_cap * pitch_of(plan.cols));
    int32_t *hmin = kh + plan.cols * ksz_h, *hn = hmin + plan.cols;
    int32_t *kv = hn + plan.cols;
    int32_t *vmin = kv + plan.rows * ksz_v, *vn = vmin + plan.rows;

    // output rows of the tile that show the resampled image: [vr0, vr1) relative to the tile
    const int vr0 = min(max(-(s.win_y + oy0), 0), nrows), vr1 = max(min(s.res_h - (s.win_y + oy0), nrows), vr0);

    const int tid = threadIdx.x;
    for (int j = tid; j < ncols + (vr1 - vr0); j += kThreads) {
        if (j < ncols) {
            const int wx = s.flip ? s.out_w - 1 - (ox0 + j) : ox0 + j;    // column of the window this output column shows
            const int rx = s.win_x + wx;
            int xmin = 0, n = 0;                                        // n = 0: outside the resampled image -> zeros
            if (rx >= 0 && rx < s.res_w) n = axis_coeffs(s.crop_w, s.res_w, s.filter, rx, kh + j * ksz_h, &xmin);
            hmin[j] = xmin;
            hn[j] = n;
        } else {
            const int r = vr0 + (j - ncols);
            int ymin;
            vn[r] = axis_coeffs(s.crop_h, s.res_h, s.filter, s.win_y + oy0 + r, kv + r * ksz_v, &ymin);
            vmin[r] = ymin;
        }
    }
    __syncthreads();

    int srow0 = 0, span = 0;
    if (vr1 > vr0) {
        srow0 = vmin[vr0];
        span = vmin[vr1 - 1] + vn[vr1 - 1] - srow0;
    }
    if (span > plan.span_cap) return;   // cannot happen for bounds from axis_bounds (span_bound); never write past the LDS

    // horizontal pass: (source row, tile column) -> 3 bytes of the intermediate
    const uint8_t *img = src + s.src_offset + (int64_t)s.crop_y * s.src_row_bytes + 3 * (int64_t)s.crop_x;
    // (thread -> column, row) by shift and mask: the column count rounded up to a power of two
    const int csh = ceil_log2(ncols);
    for (int item = tid; (item >> csh) < span; item += kThreads) {
        const int r = item >> csh, c = item & ((1 << csh) - 1);
        if (c >= ncols) continue;
        const int n = hn[c];
        const uint8_t *p = img + (int64_t)(srow0 + r) * s.src_row_bytes + 3 * hmin[c];
        const int32_t *k = kh + c * ksz_h;
        int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int x = 0; x < n; ++x) {
            const int32_t w = k[x];
            a0 += (int32_t)p[3 * x] * w;
            a1 += (int32_t)p[3 * x + 1] * w;
            a2 += (int32_t)p[3 * x + 2] * w;
        }
        uint8_t *m = mid + r * pitch + 3 * c;
        m[0] = n ? (uint8_t)clip8_byte(a0) : 0;
        m[1] = n ? (uint8_t)clip8_byte(a1) : 0;
        m[2] = n ? (uint8_t)clip8_byte(a2) : 0;
    }
    __syncthreads();

    // vertical pass: four consecutive bytes of an output row per thread
    const int groups = pitch / 4;
    const int gsh = ceil_log2(groups);
    for (int item = tid; (item >> gsh) < nrows; item += kThreads) {
        const int r = item >> gsh, g = item & ((1 << gsh) - 1);
        if (g >= groups) continue;
        uint32_t packed = 0;
        if (r >= vr0 && r < vr1) {
            const int n = vn[r];
            const uint8_t *m = mid + (vmin[r] - srow0) * pitch + 4 * g;
            const int32_t *k = kv + r * ksz_v;
            int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int y = 0; y < n; ++y) {
                const uint32_t v = *reinterpret_cast<const uint32_t *>(m + y * pitch);
                const int32_t w = k[y];
                a0 += (int32_t)(v & 0xff) * w;
                a1 += (int32_t)((v >> 8) & 0xff) * w;
                a2 += (int32_t)((v >> 16) & 0xff) * w;
                a3 += (int32_t)(v >> 24) * w;
            }
            packed = clip8_byte(a0) | (clip8_byte(a1) << 8) | (clip8_byte(a2) << 16) | (clip8_byte(a3) << 24);
        }
        uint8_t *o = dst + s.dst_offset + (int64_t)(oy0 + r) * s.dst_row_bytes + 3 * (int64_t)ox0 + 4 * g;
        const int left = row_bytes - 4 * g;          // bytes of this group inside the tile's row (the pitch pads to 4)
        if (left >= 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(o) = packed;
        } else {
            for (int b = 0; b < min(left, 4); ++b) o[b] = (uint8_t)(packed >> (8 * b));
        }
    }
}

}  // namespace
}  // namespace wv

extern "C" int wv_image_size(const uint8_t *src, uint8_t *dst, const wv_size_stage *stages, int n, int max_out_h, int max_out_w,
                             int max_ksize, void *stream)
{
    using namespace wv::isz;
    WV_REQUIRE(n >= 0, "wv_image_size: n = %d is negative", n);
    if (n == 0) return WV_OK;
    WV_REQUIRE(src && dst && stages, "wv_image_size: src / dst / stages is NULL");
    WV_REQUIRE(max_out_h >= 1 && max_out_w >= 1 && max_ksize >= 1, "wv_image_size: max_out_h = %d, max_out_w = %d, max_ksize = %d (all >= 1)",
               max_out_h, max_out_w, max_ksize);
    if (max_out_h > wv::kMaxImageSide || max_out_w > wv::kMaxImageSide)
        WV_FAIL(WV_ENOTSUP, "wv_image_size: max_out_h = %d, max_out_w = %d (limit %d)", max_out_h, max_out_w, wv::kMaxImageSide);
    if (max_ksize > kMaxKsize) WV_FAIL(WV_ENOTSUP, "wv_image_size: max_ksize = %d (limit %d: a down-scale of %d)", max_ksize, kMaxKsize, kMaxDownscale);
    // LDS: what the largest tile needs at these tap counts, inside [kMinLds, kMaxLds]; every image then plans its own tile
    // under that budget, never smaller than the tile of (max_ksize, max_ksize), which sizes the grid
    size_t lds = lds_need(16, 256, max_ksize, max_ksize);
    lds = std::min(std::max(lds, kMinLds), kMaxLds);
    const TilePlan worst = tile_plan(max_ksize, max_ksize, lds);
    if (worst.rows == 0) WV_FAIL(WV_ENOTSUP, "wv_image_size: no tile fits %zu bytes of LDS at max_ksize = %d", lds, max_ksize);
    const int64_t tiles = wv::ceil_div(max_out_h, worst.rows) * wv::ceil_div(max_out_w, worst.cols);
    if (tiles > 0x7fffffff) WV_FAIL(WV_ENOTSUP, "wv_image_size: %lld tiles per image", (long long)tiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wv::image_size_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) WV_FAIL(WV_EHIP, "wv_image_size: LDS attribute: %s", hipGetErrorString(e));
    }
    for (int i0 = 0; i0 < n; i0 += 65535) {
        const int cnt = std::min(65535, n - i0);
        hipLaunchKernelGGL(wv::image_size_kernel, dim3((unsigned)tiles, (unsigned)cnt), dim3(wv::kThreads), lds, st, src, dst, stages + i0, (int)lds);
        WV_CHECK_LAUNCH("wv_image_size");
    }
    return WV_OK;
}
