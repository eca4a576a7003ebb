// Host twin of the grouped LayerNorm kernel (group_layernorm.hip) and the one argument check of both: HOST pointers, no HIP
// call, no thread, no global state.  The twin replays the kernel's 64 lanes and its xor butterfly in a loop with the
// functions of group_layernorm.hpp: the two agree bit for bit.
#include <math.h>
#include <stdint.h>

#include "group_layernorm.hpp"

namespace {

using namespace wv::gln;

// what the 64 lanes hold after `v += v of lane ^ d` for d = 32 .. 1; every lane ends with the same bits -> lane 0's
float butterfly(float p[kLanes])
{
    float t[kLanes];
    for (int d = kLanes / 2; d > 0; d >>= 1) {
        for (int l = 0; l < kLanes; ++l) t[l] = p[l] + p[l ^ d];
        for (int l = 0; l < kLanes; ++l) p[l] = t[l];
    }
    return p[0];
}

template <class TI, class TO>
void run_rows(const TI *x, TO *out, int64_t N, int64_t T, int E, int G, const float *gamma, const float *beta, float eps)
{
    const int V = vec_of(E);
    const int64_t chunk = group_chunk(N, G);
    for (int64_t n = 0; n < N; ++n) {
        const float *gm = gamma + (n / chunk) * E, *bt = beta + (n / chunk) * E;
        for (int64_t t = 0; t < T; ++t) {
            const TI *xr = x + (n * T + t) * E;
            TO *yr = out + (n * T + t) * E;
            float p[kLanes];
            for (int lane = 0; lane < kLanes; ++lane) {
                float s = 0.f;
                for_lane_accesses(E, V, lane, [&](int c) {
                    for (int i = 0; i < V; ++i) s = add_value(s, load_value(xr + c + i));
                });
                p[lane] = s;
            }
            const float mean = mean_of(butterfly(p), E);
            for (int lane = 0; lane < kLanes; ++lane) {
                float q = 0.f;
                for_lane_accesses(E, V, lane, [&](int c) {
                    for (int i = 0; i < V; ++i) q = add_square(q, load_value(xr + c + i), mean);
                });
                p[lane] = q;
            }
            const float rstd = rstd_of(butterfly(p), E, eps);
            for (int e = 0; e < E; ++e) store_value(yr + e, affine(load_value(xr + e), mean, rstd, gm[e], bt[e]));
        }
    }
}

bool known_dtype(int dt) { return dt == WV_DT_F32 || dt == WV_DT_BF16; }

}  // namespace

int wv::gln::check_pointers(const char *what, const void *x, const void *out, const float *gamma, const float *beta)
{
    if (!x) WV_FAIL(WV_EINVAL, "%s: x is NULL", what);
    if (!out) WV_FAIL(WV_EINVAL, "%s: out is NULL", what);
    if (!gamma) WV_FAIL(WV_EINVAL, "%s: gamma is NULL", what);
    if (!beta) WV_FAIL(WV_EINVAL, "%s: beta is NULL", what);
    if (out == x) WV_FAIL(WV_EINVAL, "%s: out == x (the passes re-read x: not in place)", what);
    return WV_OK;
}

extern "C" int wv_group_layernorm_check(int x_dtype, int out_dtype, int64_t N, int64_t T, int E, int G)
{
    if (!known_dtype(x_dtype)) WV_FAIL(WV_EINVAL, "wv_group_layernorm: x_dtype = %d (WV_DT_F32 or WV_DT_BF16)", x_dtype);
    if (!known_dtype(out_dtype)) WV_FAIL(WV_EINVAL, "wv_group_layernorm: out_dtype = %d (WV_DT_F32 or WV_DT_BF16)", out_dtype);
    if (N < 0) WV_FAIL(WV_EINVAL, "wv_group_layernorm: N = %lld is negative", (long long)N);
    if (T < 0) WV_FAIL(WV_EINVAL, "wv_group_layernorm: T = %lld is negative", (long long)T);
    if (E < 1) WV_FAIL(WV_EINVAL, "wv_group_layernorm: E = %d (must be >= 1)", E);
    if (G < 1) WV_FAIL(WV_EINVAL, "wv_group_layernorm: G = %d (must be >= 1)", G);
    const int64_t max_rows = 4 * (int64_t)INT32_MAX;              // one wave per row, four per workgroup, grid.x < 2^31
    if (N > 0 && T > max_rows / N)
        WV_FAIL(WV_ENOTSUP, "wv_group_layernorm: N * T = %lld * %lld rows (limit %lld)", (long long)N, (long long)T, (long long)max_rows);
    return WV_OK;
}

extern "C" int wv_group_layernorm_cpu(const void *x, int x_dtype, void *out, int out_dtype, int64_t N, int64_t T, int E, int G,
                                      const float *gamma, const float *beta, float eps)
{
    int rc = wv_group_layernorm_check(x_dtype, out_dtype, N, T, E, G);
    if (rc != WV_OK) return rc;
    if (N * T == 0) return WV_OK;
    rc = check_pointers("wv_group_layernorm_cpu", x, out, gamma, beta);
    if (rc != WV_OK) return rc;
    const bool xf = x_dtype == WV_DT_F32, of = out_dtype == WV_DT_F32;
    const float *x32 = static_cast<const float *>(x);
    const uint16_t *x16 = static_cast<const uint16_t *>(x);
    float *o32 = static_cast<float *>(out);
    uint16_t *o16 = static_cast<uint16_t *>(out);
    if (xf && of) run_rows(x32, o32, N, T, E, G, gamma, beta, eps);
    else if (xf) run_rows(x32, o16, N, T, E, G, gamma, beta, eps);
    else if (of) run_rows(x16, o32, N, T, E, G, gamma, beta, eps);
    else run_rows(x16, o16, N, T, E, G, gamma, beta, eps);
    return WV_OK;
}
