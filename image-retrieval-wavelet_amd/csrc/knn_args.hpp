// What wv_knn_float / wv_rank_scores (knn_float.hip) and their host twins (host_knn.cpp) share: the argument rules -- every
// refusal is answered here, before any pointer is read and before any HIP call -- and the order-preserving key of a score.
// No HIP header is included, so a plain C++ compiler can take this file; under hipcc (__HIP__) the two key functions are
// __host__ __device__ and always inlined (WV_HD): knn_float.hip compiles them into its kernels.
#pragma once
#include <stdint.h>

#include "twin.hpp"

namespace wv {

constexpr int64_t kKnnMaxN = 1ll << 26;   // the kernels' 32-bit byte offsets into a score row block

// wv_knn_float[_cpu].  what: the entry point's name in the message
inline int knn_float_args(const char *what, bool buffers, int Q, int64_t N, int D, int metric, int k)
{
    if (!buffers) WV_FAIL(WV_EINVAL, "%s: null buffer", what);
    if (!(Q >= 0 && N >= 1 && D >= 1)) WV_FAIL(WV_EINVAL, "%s: bad shape Q=%d N=%lld D=%d", what, Q, (long long)N, D);
    if (!(metric == WV_METRIC_IP || metric == WV_METRIC_L2 || metric == WV_METRIC_L2_SQUARED))
        WV_FAIL(WV_EINVAL, "%s: metric %d", what, metric);
    if (!(k >= 1 && k <= N)) WV_FAIL(WV_EINVAL, "%s: k=%d must be in [1, N=%lld] (torch.topk raises too)", what, k, (long long)N);
    if (N > kKnnMaxN) WV_FAIL(WV_EINVAL, "%s: N=%lld above the supported 2^26 rows", what, (long long)N);
    return WV_OK;
}

// wv_rank_scores[_cpu]
inline int rank_scores_args(const char *what, bool buffers, int Q, int64_t N, int k, int flags)
{
    if (!buffers) WV_FAIL(WV_EINVAL, "%s: null buffer", what);
    if (!(Q >= 0 && N >= 1)) WV_FAIL(WV_EINVAL, "%s: bad shape Q=%d N=%lld", what, Q, (long long)N);
    if (!(k >= 1 && k <= N)) WV_FAIL(WV_EINVAL, "%s: k=%d must be in [1, N=%lld]", what, k, (long long)N);
    if (N > kKnnMaxN) WV_FAIL(WV_EINVAL, "%s: N=%lld above the supported 2^26 columns", what, (long long)N);
    if ((flags & ~(WV_RANK_DESCENDING | WV_RANK_SQRT)) != 0) WV_FAIL(WV_EINVAL, "%s: flags %d", what, flags);
    return WV_OK;
}

// 32-bit image of a score whose unsigned order is the ranking order: ascending float order (-0 = +0), descending: reversed
WV_HD __attribute__((always_inline)) uint32_t float_to_key(float v, bool descending)
{
    v += 0.0f;  // -0 -> +0
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;  // ascending float order -> ascending unsigned
    return descending ? ~u : u;
}
WV_HD __attribute__((always_inline)) float key_to_float(uint32_t u, bool descending)
{
    if (descending) u = ~u;
    u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}

}  // namespace wv
