// Grouped LayerNorm on the GPU (include/wvhash.h: wv_group_layernorm): torch.chunk(G, 0) -> one nn.LayerNorm per chunk ->
// torch.cat as ONE pass over [N][T][E]: x is read once and out written once, in fp32 or bf16 on either side.  The arithmetic
// and the order of the sums are group_layernorm.hpp's, which the host twin compiles too.
//
// One wave per row, four rows per 256-thread workgroup, no LDS.  An access is V = vec_of(E) consecutive values of one lane:
// for E % 4 == 0 a 16-byte (fp32) or 8-byte (bf16) load or store, so that a wave instruction covers 1 KiB (512 B) of one row
// without a gap; otherwise single values.  Rows of E <= 512 are held in registers between the three passes (sum, squares,
// affine: NJ accesses per lane); longer rows are read again from the cache by the same lane (NJ = 0).
// `wide`: every pointer is aligned for the V-wide access; when one is not, the same values move one by one.
// A wave reads and writes only the E values of its own row < N * T, and gamma / beta of its group < G.
#include "group_layernorm.hpp"
#include "common.hpp"

namespace wv {
namespace {

using namespace gln;

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / kWave;

template <int V>
__device__ __forceinline__ void load_access(const float *p, bool wide, float v[V])
{
    if constexpr (V == 4) {
        if (wide) {
            const float4 t = *reinterpret_cast<const float4 *>(p);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = p[i];
}

template <int V>
__device__ __forceinline__ void load_access(const uint16_t *p, bool wide, float v[V])
{
    if constexpr (V == 4) {
        if (wide) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p);
            v[0] = __uint_as_float(t.x << 16), v[1] = __uint_as_float(t.x & 0xffff0000u);
            v[2] = __uint_as_float(t.y << 16), v[3] = __uint_as_float(t.y & 0xffff0000u);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = widen_bf16(p[i]);
}

template <int V>
__device__ __forceinline__ void store_access(float *p, bool wide, const float v[V])
{
    if constexpr (V == 4) {
        if (wide) {
            *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = v[i];
}

template <int V>
__device__ __forceinline__ void store_access(uint16_t *p, bool wide, const float v[V])
{
    if constexpr (V == 4) {
        if (wide) {
            uint2 t;
            t.x = (uint32_t)round_bf16(v[0]) | ((uint32_t)round_bf16(v[1]) << 16);
            t.y = (uint32_t)round_bf16(v[2]) | ((uint32_t)round_bf16(v[3]) << 16);
            *reinterpret_cast<uint2 *>(p) = t;
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = round_bf16(v[i]);
}

__device__ __forceinline__ float butterfly(float v)
{
#pragma unroll
    for (int d = kLanes / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kLanes);
    return v;
}

template <int V, int NJ, class TI, class TO>
__global__ __launch_bounds__(kThreads) void group_layernorm_kernel(const TI *__restrict__ x, TO *__restrict__ out, int64_t rows,
                                                                   int64_t T, int E, int64_t chunk,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, float eps, int wide_flag)
{
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave_id();
    if (row >= rows) return;
    const bool wide = wide_flag != 0;
    const TI *xr = x + row * E;
    TO *yr = out + row * E;
    const int64_t group = (row / T) / chunk;
    const float *gm = gamma + group * E, *bt = beta + group * E;
    constexpr int kStep = kLanes * V;

    float val[NJ > 0 ? NJ : 1][V];
    float s = 0.f;
    if constexpr (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane * V + j * kStep;
            if (c < E) {
                load_access<V>(xr + c, wide, val[j]);
#pragma unroll
                for (int i = 0; i < V; ++i) s = add_value(s, val[j][i]);
            }
        }
    } else {
        for_lane_accesses(E, V, lane, [&](int c) {
            float v[V];
            load_access<V>(xr + c, wide, v);
#pragma unroll
            for (int i = 0; i < V; ++i) s = add_value(s, v[i]);
        });
    }
    const float mean = mean_of(butterfly(s), E);

    float q = 0.f;
    if constexpr (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (lane * V + j * kStep < E) {
#pragma unroll
                for (int i = 0; i < V; ++i) q = add_square(q, val[j][i], mean);
            }
        }
    } else {
        for_lane_accesses(E, V, lane, [&](int c) {
            float v[V];
            load_access<V>(xr + c, wide, v);
#pragma unroll
            for (int i = 0; i < V; ++i) q = add_square(q, v[i], mean);
        });
    }
    const float rstd = rstd_of(butterfly(q), E, eps);

    auto emit = [&](int c, const float v[V]) {
        float g[V], b[V], y[V];
        load_access<V>(gm + c, wide, g);
        load_access<V>(bt + c, wide, b);
#pragma unroll
        for (int i = 0; i < V; ++i) y[i] = affine(v[i], mean, rstd, g[i], b[i]);
        store_access<V>(yr + c, wide, y);
    };
    if constexpr (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane * V + j * kStep;
            if (c < E) emit(c, val[j]);
        }
    } else {
        for_lane_accesses(E, V, lane, [&](int c) {
            float v[V];
            load_access<V>(xr + c, wide, v);
            emit(c, v);
        });
    }
}

template <class TI, class TO>
void launch(const TI *x, TO *out, int64_t rows, int64_t T, int E, int64_t chunk, const float *gamma, const float *beta, float eps,
            hipStream_t st)
{
    const int V = vec_of(E);
    const uintptr_t bits = (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(TI) - 1)) | (reinterpret_cast<uintptr_t>(out) & (4 * sizeof(TO) - 1)) |
                           ((reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15);
    const int wide = V == 4 && bits == 0;
    const dim3 grid((unsigned)ceil_div(rows, kRowsPerBlock)), block(kThreads);
    const bool regs = E <= kRegE;
#define WV_GLN_LAUNCH(V_, NJ_) \
    hipLaunchKernelGGL((group_layernorm_kernel<V_, NJ_, TI, TO>), grid, block, 0, st, x, out, rows, T, E, chunk, gamma, beta, eps, wide)
    if (V == 4 && regs) WV_GLN_LAUNCH(4, kRegE / (kLanes * 4));
    else if (V == 4) WV_GLN_LAUNCH(4, 0);
    else if (regs) WV_GLN_LAUNCH(1, kRegE / kLanes);
    else WV_GLN_LAUNCH(1, 0);
#undef WV_GLN_LAUNCH
}

}  // namespace
}  // namespace wv

extern "C" int wv_group_layernorm(const void *x, int x_dtype, void *out, int out_dtype, int64_t N, int64_t T, int E, int G,
                                  const float *gamma, const float *beta, float eps, void *stream)
{
    int rc = wv_group_layernorm_check(x_dtype, out_dtype, N, T, E, G);
    if (rc != WV_OK) return rc;
    const int64_t rows = N * T;
    if (rows == 0) return WV_OK;
    rc = wv::gln::check_pointers("wv_group_layernorm", x, out, gamma, beta);
    if (rc != WV_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t chunk = wv::gln::group_chunk(N, G);
    const bool xf = x_dtype == WV_DT_F32, of = out_dtype == WV_DT_F32;
    const float *x32 = static_cast<const float *>(x);
    const uint16_t *x16 = static_cast<const uint16_t *>(x);
    float *o32 = static_cast<float *>(out);
    uint16_t *o16 = static_cast<uint16_t *>(out);
    if (xf && of) wv::launch(x32, o32, rows, T, E, chunk, gamma, beta, eps, st);
    else if (xf) wv::launch(x32, o16, rows, T, E, chunk, gamma, beta, eps, st);
    else if (of) wv::launch(x16, o32, rows, T, E, chunk, gamma, beta, eps, st);
    else wv::launch(x16, o16, rows, T, E, chunk, gamma, beta, eps, st);
    WV_CHECK_LAUNCH("wv_group_layernorm");
    return WV_OK;
}
