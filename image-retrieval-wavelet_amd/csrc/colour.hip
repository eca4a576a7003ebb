// Colour jitter on the GPU: brightness / contrast / saturation in a per-image order, in place on a ragged batch of 3-channel
// uint8 HWC images (include/wvhash.h: wv_colour_jitter).  Pillow's ImageEnhance restated (colour.hpp) -- the per-pixel chain
// is the function the host twin compiles too.
//
// Both launches: grid = (tiles, images), 256 threads.  An image is h x ceil(w / 4) groups of four pixels (12 bytes); a tile
// is kTileGroups consecutive groups in row-major order, a thread takes every 256th of them, so that a wave reads 768
// consecutive bytes of a row.  A full group whose first byte is dword-aligned moves as three dwords; any other (row starts of
// odd offsets or pitches, the last pixels of a row whose width is no multiple of four) moves byte by byte.
//   1. statistics: only for images whose chain has contrast.  The operations in front of contrast are pointwise and run on
//      the fly; L of every pixel is summed: per thread in 32 bits (16 pixels), over the wave by shuffles, over the workgroup
//      through LDS, then ONE atomicAdd of the workgroup's sum onto the image's 64-bit sum.  Integer sums: any order, one result.
//   2. apply: reads the descriptor and the sum, derives the contrast mean, runs the whole chain per pixel, writes in place.
// Everything a thread writes lies inside the 3 * w bytes of one of its image's h rows.
#include "colour.hpp"
#include "common.hpp"

namespace wv {
namespace {

using namespace col;

constexpr int kThreads = 256;
constexpr int kGroupsPerThread = 4;
constexpr int kTileGroups = kThreads * kGroupsPerThread;

struct Group {
    uint8_t *p;      // first byte of the group
    int pixels;      // 1..4
    bool wide;       // three aligned dwords
};

__device__ __forceinline__ Group group_of(uint8_t *img, const wv_colour_ops &o, int groups_per_row, int item)
{
    Group g;
    const int y = item / groups_per_row, gx = item - y * groups_per_row;
    g.p = img + o.offset + (int64_t)y * o.row_bytes + 12 * (int64_t)gx;
    g.pixels = min(4, o.w - 4 * gx);
    g.wide = g.pixels == 4 && (reinterpret_cast<uintptr_t>(g.p) & 3) == 0;
    return g;
}

__device__ __forceinline__ void load_group(const Group &g, uint32_t v[3])
{
    if (g.wide) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(g.p);
        v[0] = q[0];
        v[1] = q[1];
        v[2] = q[2];
    } else {
        v[0] = v[1] = v[2] = 0;
#pragma unroll
        for (int b = 0; b < 12; ++b)
            if (b < 3 * g.pixels) v[b >> 2] |= (uint32_t)g.p[b] << (8 * (b & 3));
    }
}

__device__ __forceinline__ int byte_of(const uint32_t v[3], int b) { return (int)((v[b >> 2] >> (8 * (b & 3))) & 0xff); }

__global__ __launch_bounds__(kThreads) void colour_stats_kernel(uint8_t *__restrict__ img, const wv_colour_ops *__restrict__ ops,
                                                                unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t part[kThreads / kWave];
    const wv_colour_ops o = ops[blockIdx.y];
    const int cpos = contrast_index(o);
    if (cpos < 0) return;
    const int gpr = (o.w + 3) >> 2;
    const int items = o.h * gpr;                       // <= 16384 * 4096
    const int first = (int)blockIdx.x * kTileGroups;
    if (first >= items) return;
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerThread; ++k) {
        const int item = first + k * kThreads + (int)threadIdx.x;
        if (item >= items) break;
        const Group g = group_of(img, o, gpr, item);
        uint32_t v[3];
        load_group(g, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= g.pixels) break;
            int r = byte_of(v, 3 * j), gg = byte_of(v, 3 * j + 1), b = byte_of(v, 3 * j + 2);
            run_ops(o, 0, cpos, 0, &r, &gg, &b);
            acc += (uint32_t)luma(r, gg, b);
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < kThreads / kWave; ++i) total += part[i];
        atomicAdd(&sums[blockIdx.y], total);
    }
}

__global__ __launch_bounds__(kThreads) void colour_apply_kernel(uint8_t *__restrict__ img, const wv_colour_ops *__restrict__ ops,
                                                                const unsigned long long *__restrict__ sums)
{
    const wv_colour_ops o = ops[blockIdx.y];
    const int n_ops = op_count(o);
    if (n_ops == 0) return;
    const int gpr = (o.w + 3) >> 2;
    const int items = o.h * gpr;
    const int first = (int)blockIdx.x * kTileGroups;
    if (first >= items) return;
    __shared__ int mean;                               // one 64-bit division per workgroup
    if (threadIdx.x == 0) mean = contrast_index(o) >= 0 ? mean_from_sum(sums[blockIdx.y], (uint64_t)o.h * (uint64_t)o.w) : 0;
    __syncthreads();
    const int m = mean;
#pragma unroll
    for (int k = 0; k < kGroupsPerThread; ++k) {
        const int item = first + k * kThreads + (int)threadIdx.x;
        if (item >= items) break;
        const Group g = group_of(img, o, gpr, item);
        uint32_t v[3], out[3] = {0, 0, 0};
        load_group(g, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= g.pixels) break;
            int r = byte_of(v, 3 * j), gg = byte_of(v, 3 * j + 1), b = byte_of(v, 3 * j + 2);
            run_ops(o, 0, n_ops, m, &r, &gg, &b);
            out[(3 * j) >> 2] |= own_byte(r) << (8 * ((3 * j) & 3));
            out[(3 * j + 1) >> 2] |= own_byte(gg) << (8 * ((3 * j + 1) & 3));
            out[(3 * j + 2) >> 2] |= own_byte(b) << (8 * ((3 * j + 2) & 3));
        }
        if (g.wide) {
            uint32_t *q = reinterpret_cast<uint32_t *>(g.p);
            q[0] = out[0];
            q[1] = out[1];
            q[2] = out[2];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < 3 * g.pixels) g.p[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
        }
    }
}

}  // namespace
}  // namespace wv

extern "C" size_t wv_colour_jitter_workspace_bytes(int n) { return n > 0 ? (size_t)n * sizeof(unsigned long long) : 0; }

extern "C" int wv_colour_jitter(uint8_t *img, const wv_colour_ops *ops, int n, int max_h, int max_w, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    using namespace wv::col;
    WV_REQUIRE(n >= 0, "wv_colour_jitter: n = %d is negative", n);
    if (n == 0) return WV_OK;
    WV_REQUIRE(img && ops, "wv_colour_jitter: img / ops is NULL");
    WV_REQUIRE(max_h >= 1 && max_w >= 1, "wv_colour_jitter: max_h = %d, max_w = %d (both >= 1)", max_h, max_w);
    if (max_h > wv::kMaxImageSide || max_w > wv::kMaxImageSide)
        WV_FAIL(WV_ENOTSUP, "wv_colour_jitter: max_h = %d, max_w = %d (limit %d)", max_h, max_w, wv::kMaxImageSide);
    const size_t need = wv_colour_jitter_workspace_bytes(n);
    WV_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "wv_colour_jitter: workspace is NULL or not 8-byte aligned");
    if (workspace_bytes < need) WV_FAIL(WV_ENOMEM, "wv_colour_jitter: workspace_bytes = %zu, need %zu", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long *sums = static_cast<unsigned long long *>(workspace);
    hipError_t e = hipMemsetAsync(sums, 0, need, st);
    if (e != hipSuccess) WV_FAIL(WV_EHIP, "wv_colour_jitter: clearing the workspace: %s", hipGetErrorString(e));
    const int64_t tiles = wv::ceil_div((int64_t)max_h * ((max_w + 3) / 4), wv::kTileGroups);   // <= 65536
    for (int pass = 0; pass < 2; ++pass) {
        for (int i0 = 0; i0 < n; i0 += 65535) {
            const dim3 grid((unsigned)tiles, (unsigned)std::min(65535, n - i0));
            if (pass == 0)
                hipLaunchKernelGGL(wv::colour_stats_kernel, grid, dim3(wv::kThreads), 0, st, img, ops + i0, sums + i0);
            else
                hipLaunchKernelGGL(wv::colour_apply_kernel, grid, dim3(wv::kThreads), 0, st, img, ops + i0, sums + i0);
            WV_CHECK_LAUNCH("wv_colour_jitter");
        }
    }
    return WV_OK;
}
