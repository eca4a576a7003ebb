// ToTensor -> Normalize -> CustomTransform for a whole batch on gfx950 (include/wvhash.h: wv_lift_images): the sized uint8
// batch in, the coarsest lifting bands out, bit-identical to the reference's float32 torch ops.  The conversion and the
// lifting chain are lifting.hpp's, the functions the host twin (host_lifting.cpp) compiles too.
//
// ONE launch per level over the whole batch, both passes in it.  grid = (units, tile rows, tile columns), 256 threads.  A
// workgroup owns kTilePairsH x kTilePairsW (8 x 64) output samples of every band of one plane, i.e. 16 x 128 input samples;
// cdf 9/7 adds a halo of 4 samples on every side (output pair i reads samples 2i - 4 .. 2i + 4) and recomputes the
// intermediates in it, haar needs none.  Per tile:
//   1. level 1 of a uint8 batch: the tile's bytes are staged in LDS as aligned dwords, row by row -- with NHWC input once for
//      all channels (a unit is an image, the channels loop inside the workgroup), with NCHW input per plane (a unit is a
//      plane).  A dword that would reach outside the tensor is assembled from bytes.
//   2. the tile as fp32 in LDS: bytes through the 256 x C table (built per workgroup from lifting.hpp's convert_byte), fp32
//      sources (float input, the LL planes of the previous level) directly.  A sample beyond H or W is +0.0: the pads of
//      HaarLifting / Cdf97Lifting are never made in memory.
//   3. H pass on every column of the tile (halo columns included) -> `mid`: s rows, then d rows, even and odd columns apart
//      and laid out for the W pass (mid_at).  A thread takes a run of four pairs of its column: neighbouring pairs share the
//      intermediates of the cdf 9/7 chain (lift::pairs), which are then formed once per run, not once per pair.
//   4. W pass, a run of four pairs of a row per thread -> LL (x 1/2), HL | LH, HH (x sqrt 2) stored straight to their place,
//      16 bytes at a time where the run is whole and aligned: a non-final level stores LL alone into the workspace (the
//      detail bands are never formed), the final level writes the requested bands into `out`.
// The zero-for-outside rule of the lifting steps is evaluated with IMAGE coordinates (pair index against the plane's pair
// count), never with tile coordinates: a tile edge inside the image reads its halo.
// Everything a thread stores lies inside its plane's nh x nw samples of a band; every load is guarded by the plane's h x w.
#include "common.hpp"
#include "lifting.hpp"

#pragma clang fp contract(off)

namespace wv {
namespace {

using namespace lift;

constexpr int kThreads = 256;
// A row of `mid` holds the H-pass results of the tile's columns by column PAIR p: the even columns at mid_at(p), the odd ones
// kMidStride words behind.  Pair p lies at (p % 4) * kMidQuarter + p / 4, so that the W pass, whose lanes take runs of four
// pairs, reads consecutive words with consecutive lanes; with quarters 20 and halves 80 words apart, the eight groups a
// half-wave of the H pass stores to (4 quarters x even / odd) fall on eight disjoint sets of four banks.
constexpr int kMidQuarter = 20, kMidStride = 4 * kMidQuarter;
__device__ __forceinline__ int mid_at(int p) { return (p & 3) * kMidQuarter + (p >> 2); }

constexpr int kRun = 4;             // consecutive pairs per thread and pass: they share the intermediates of the cdf 9/7 chain
static_assert(kTilePairsH % kRun == 0 && kTilePairsW % kRun == 0, "a tile is whole runs");

// `count` (1 .. kRun) consecutive samples of a band row: one 16-byte store where the run is whole and aligned
__device__ __forceinline__ void store_run(float *p, const float (&v)[kRun], int count)
{
    static_assert(kRun == 4, "float4");
    if (count == kRun && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < kRun; ++u)
            if (u < count) p[u] = v[u];
    }
}

struct LevelArgs {
    const void *src;
    float *dst;
    int64_t src_bytes;              // uint8 source: size of the tensor, the window whole dwords may be read from
    int64_t s_img, s_ch, s_y, s_x;  // source strides in elements
    int C, cpb;                     // channels of the batch; channels per unit: C (a unit is an image) or 1 (a plane)
    int h, w;                       // source plane, unpadded
    int nh, nw;                     // pairs per axis = size of a band
    int bands;                      // stored per plane: 1 = LL, 4 = LL, LH, HL, HH
    Consts k;
    Convert cv;
};

template <int BASIS, bool U8>
__global__ __launch_bounds__(kThreads) void lift_level_kernel(const LevelArgs a)
{
    constexpr int HALO = BASIS == kCdf97 ? 2 * kHaloPairs : 0;       // samples on each side
    constexpr int TH = kTilePairsH, TW = kTilePairsW;
    constexpr int R = 2 * TH + 2 * HALO, CN = 2 * TW + 2 * HALO;
    constexpr int ND = U8 ? (CN * kMaxChannels + 6) / 4 : 1;         // dwords of a staged row: its bytes + up to 3 + 3 of alignment
    static_assert(TW + HALO <= 4 * kMidQuarter, "mid row");
    __shared__ float tile[R][CN];
    __shared__ float mid[2 * TH][2 * kMidStride];
    __shared__ uint32_t raw[U8 ? R : 1][ND];
    __shared__ float table[U8 ? kMaxChannels * 256 : 1];

    const int tid = threadIdx.x;
    const int unit = blockIdx.x, i0 = (int)blockIdx.y * TH, j0 = (int)blockIdx.z * TW;
    const int y0 = 2 * i0 - HALO, x0 = 2 * j0 - HALO;
    const int64_t img = a.cpb == 1 ? unit / a.C : unit;
    const int c_first = a.cpb == 1 ? unit % a.C : 0;
    const int ya = max(y0, 0), yb = min(y0 + R, a.h), xa = max(x0, 0), xb = min(x0 + CN, a.w);   // the tile inside the plane

    // uint8 source: the first byte of the tile's row y0 + r sits (align0 + r * pitch3) % 4 bytes into its first staged dword
    int align0 = 0, pitch3 = 0;
    if constexpr (U8) {
        const uintptr_t first0 = reinterpret_cast<uintptr_t>(a.src) + (uintptr_t)(img * a.s_img + (a.cpb == 1 ? c_first * a.s_ch : 0) +
                                                                                  (int64_t)y0 * a.s_y + (int64_t)xa * a.s_x);
        align0 = (int)(first0 & 3), pitch3 = (int)(a.s_y & 3);
        for (int e = tid; e < a.C * 256; e += kThreads) table[e] = convert_byte(a.cv, e >> 8, e & 255);
        const uint8_t *lo = static_cast<const uint8_t *>(a.src), *hi = lo + a.src_bytes;
        const uint8_t *base = lo + img * a.s_img + (a.cpb == 1 ? c_first * a.s_ch : 0);
        const int seg = (xb - xa) * (int)a.s_x;                       // bytes of a row inside the tile (<= CN * C)
        for (int e = tid; e < (yb - ya) * ND; e += kThreads) {
            const int r = e / ND, k = e - r * ND;
            const uint8_t *first = base + (int64_t)(ya + r) * a.s_y + (int64_t)xa * a.s_x;
            const uint8_t *p = first - (reinterpret_cast<uintptr_t>(first) & 3) + 4 * k;
            if (p >= first + seg) continue;
            uint32_t v = 0;
            if (p >= lo && p + 4 <= hi) {
                v = *reinterpret_cast<const uint32_t *>(p);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (p + q >= lo && p + q < hi) v |= (uint32_t)p[q] << (8 * q);
            }
            raw[ya - y0 + r][k] = v;
        }
    }

    for (int cc = 0; cc < a.cpb; ++cc) {
        const int c = c_first + cc;
        __syncthreads();             // table and raw are written; the previous channel's W pass is done with mid
        // 2. the tile as fp32
        for (int e = tid; e < R * CN; e += kThreads) {
            const int r = e / CN, xx = e - r * CN;
            const int y = y0 + r, x = x0 + xx;
            float v = 0.0f;
            if (y >= ya && y < yb && x >= xa && x < xb) {
                if constexpr (U8) {
                    const int off = ((align0 + r * pitch3) & 3) + (x - xa) * (int)a.s_x + (a.cpb == 1 ? 0 : c);
                    v = table[c * 256 + reinterpret_cast<const uint8_t *>(&raw[r][0])[off]];
                } else {
                    v = static_cast<const float *>(a.src)[img * a.s_img + c * a.s_ch + (int64_t)y * a.s_y + (int64_t)x * a.s_x];
                }
            }
            tile[r][xx] = v;
        }
        __syncthreads();
        // 3. H pass: pairs i .. i + 3 of column xx; the signal is the plane's column, the zero rule the plane's nh
        for (int e = tid; e < (TH / kRun) * CN; e += kThreads) {
            const int g = e / CN, xx = e - g * CN;
            const int i = i0 + g * kRun;
            if (i >= a.nh) continue;
            float s[kRun], d[kRun];
            pairs<BASIS, kRun>([&](int j) { return tile[2 * j - y0][xx]; }, [&](int j) { return tile[2 * j + 1 - y0][xx]; }, a.nh, i, a.k, s, d);
            const int at = (xx & 1) * kMidStride + mid_at(xx >> 1);
#pragma unroll
            for (int u = 0; u < kRun; ++u) {                // rows at or beyond nh hold what the zero rule yields; never read
                mid[g * kRun + u][at] = s[u];
                mid[TH + g * kRun + u][at] = d[u];
            }
        }
        __syncthreads();
        // 4. W pass: pairs j .. j + 3 of row `row` of mid (a wave holds four rows, all s or all d: that branch is wave-uniform)
        const int64_t band = (int64_t)a.nh * a.nw;
        float *plane = a.dst + (img * a.C + c) * a.bands * band;
        for (int e = tid; e < 2 * TH * (TW / kRun); e += kThreads) {
            const int row = e / (TW / kRun), jl = (e - row * (TW / kRun)) * kRun;
            const bool srow = row < TH;
            const int i = i0 + (srow ? row : row - TH), j = j0 + jl;
            if (i >= a.nh || j >= a.nw || (!srow && a.bands == 1)) continue;
            const int shift = jl + HALO / 2 - j;                                                // pair q of the row at [q + shift]
            float s[kRun], d[kRun];
            pairs<BASIS, kRun>([&](int q) { return mid[row][mid_at(q + shift)]; }, [&](int q) { return mid[row][kMidStride + mid_at(q + shift)]; },
                               a.nw, j, a.k, s, d);
#pragma unroll
            for (int u = 0; u < kRun; ++u) {
                s[u] = srow ? s[u] * a.k.sc_ll : s[u];
                d[u] = srow ? d[u] : d[u] * a.k.sc_hh;
            }
            const int64_t o = (int64_t)i * a.nw + j;
            const int count = min(kRun, a.nw - j);
            store_run(plane + (srow ? 0 : band) + o, s, count);                                 // LL | LH
            if (a.bands == 4) store_run(plane + (srow ? 2 : 3) * band + o, d, count);           // HL | HH
        }
    }
}

// levels = 0: the conversion alone, [B][C][H][W] fp32 out.  grid-stride over the output, x fastest; the table per workgroup.
template <bool U8>
__global__ __launch_bounds__(kThreads) void lift_convert_kernel(const LevelArgs a, int64_t total)
{
    __shared__ float table[U8 ? kMaxChannels * 256 : 1];
    if constexpr (U8) {
        for (int e = threadIdx.x; e < a.C * 256; e += kThreads) table[e] = convert_byte(a.cv, e >> 8, e & 255);
        __syncthreads();
    }
    const int64_t plane = (int64_t)a.h * a.w;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t p = t / plane, rest = t - p * plane;
        const int y = (int)(rest / a.w), x = (int)(rest - (int64_t)y * a.w);
        const int c = (int)(p % a.C);
        const int64_t at = (p / a.C) * a.s_img + c * a.s_ch + (int64_t)y * a.s_y + (int64_t)x * a.s_x;
        if constexpr (U8)
            a.dst[t] = table[c * 256 + static_cast<const uint8_t *>(a.src)[at]];
        else
            a.dst[t] = static_cast<const float *>(a.src)[at];
    }
}

inline size_t slot_bytes(int64_t planes, int h, int w) { return (size_t)align_up(planes * h * w * (int64_t)sizeof(float), 256); }

}  // namespace
}  // namespace wv

using namespace wv;
using namespace wv::lift;

// LL planes of level 1 (levels >= 2), then those of level 2 (levels >= 3); later levels alternate between the two slots
extern "C" size_t wv_lift_images_workspace_bytes(int B, int C, int H, int W, int basis, int levels)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (basis != kHaar && basis != kCdf97) || levels < 2 || levels > kMaxLevels) return 0;
    const int64_t planes = (int64_t)B * C;
    size_t need = slot_bytes(planes, out_size(H, basis, 1), out_size(W, basis, 1));
    if (levels >= 3) need += slot_bytes(planes, out_size(H, basis, 2), out_size(W, basis, 2));
    return need;
}

extern "C" int wv_lift_images(const void *in, int in_dtype, int in_layout, int B, int C, int H, int W, int to_tensor, const float *mean,
                              const float *std, int basis, int levels, int ll_only, float *out, void *workspace, size_t workspace_bytes,
                              void *stream)
{
    int rc = wv_lift_images_check(in_dtype, in_layout, B, C, H, W, basis, levels, ll_only);
    if (rc != WV_OK) return rc;
    LevelArgs a;
    rc = convert_args("wv_lift_images", in_dtype, C, to_tensor, mean, std, &a.cv);
    if (rc != WV_OK) return rc;
    if (B == 0) return WV_OK;
    WV_REQUIRE(in && out, "wv_lift_images: in / out is NULL");
    const size_t need = wv_lift_images_workspace_bytes(B, C, H, W, basis, levels);
    if (need) {
        WV_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "wv_lift_images: workspace is NULL or not 4-byte aligned");
        if (workspace_bytes < need) WV_FAIL(WV_ENOMEM, "wv_lift_images: workspace_bytes = %zu, need %zu", workspace_bytes, need);
    }
    WV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (in_dtype != WV_DT_F32 || (reinterpret_cast<uintptr_t>(in) & 3) == 0),
               "wv_lift_images: float32 buffers must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool u8 = in_dtype == WV_DT_U8, nhwc = in_layout == WV_LAYOUT_NHWC;
    const int64_t planes = (int64_t)B * C;
    a.k = consts(basis);
    a.C = C;
    a.src = in;
    a.src_bytes = planes * H * W;
    a.s_img = (int64_t)C * H * W;
    a.s_ch = nhwc ? 1 : (int64_t)H * W;
    a.s_y = nhwc ? (int64_t)W * C : W;
    a.s_x = nhwc ? C : 1;
    a.h = H, a.w = W;
    if (levels == 0) {
        a.dst = out, a.cpb = 1, a.nh = a.nw = 0, a.bands = 1;
        const int64_t total = planes * H * W;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(total, kThreads), 2048);
        if (u8)
            hipLaunchKernelGGL(lift_convert_kernel<true>, dim3(grid), dim3(kThreads), 0, st, a, total);
        else
            hipLaunchKernelGGL(lift_convert_kernel<false>, dim3(grid), dim3(kThreads), 0, st, a, total);
        WV_CHECK_LAUNCH("wv_lift_images");
        return WV_OK;
    }
    float *slot[2] = {static_cast<float *>(workspace), nullptr};
    if (levels >= 3) slot[1] = reinterpret_cast<float *>(static_cast<char *>(workspace) + slot_bytes(planes, out_size(H, basis, 1), out_size(W, basis, 1)));
    for (int l = 1; l <= levels; ++l) {
        const bool first = l == 1, last = l == levels, from_u8 = first && u8;
        a.nh = padded(a.h, basis) / 2, a.nw = padded(a.w, basis) / 2;
        a.dst = last ? out : slot[(l - 1) & 1];
        a.bands = last && !ll_only ? 4 : 1;
        a.cpb = from_u8 && nhwc ? C : 1;
        const dim3 grid((unsigned)(a.cpb == 1 ? planes : B), (unsigned)ceil_div(a.nh, kTilePairsH), (unsigned)ceil_div(a.nw, kTilePairsW));
        if (basis == kHaar) {
            if (from_u8)
                hipLaunchKernelGGL((lift_level_kernel<kHaar, true>), grid, dim3(kThreads), 0, st, a);
            else
                hipLaunchKernelGGL((lift_level_kernel<kHaar, false>), grid, dim3(kThreads), 0, st, a);
        } else {
            if (from_u8)
                hipLaunchKernelGGL((lift_level_kernel<kCdf97, true>), grid, dim3(kThreads), 0, st, a);
            else
                hipLaunchKernelGGL((lift_level_kernel<kCdf97, false>), grid, dim3(kThreads), 0, st, a);
        }
        WV_CHECK_LAUNCH("wv_lift_images");
        // the next level reads the LL planes just written: [planes][nh][nw] fp32
        a.src = a.dst;
        a.h = a.nh, a.w = a.nw;
        a.s_img = (int64_t)C * a.h * a.w, a.s_ch = (int64_t)a.h * a.w, a.s_y = a.w, a.s_x = 1;
    }
    return WV_OK;
}
