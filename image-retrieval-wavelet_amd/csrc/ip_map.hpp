// What wv_ip_map_at_k (ip_map.hip) and its host twin (host_ip_map.cpp) share: the limits and the argument rules -- every
// refusal is answered here, before any pointer is read and before any HIP call.  The score's accumulation order and its
// order-preserving key are wv_knn_float's (knn_args.hpp).  No HIP header is included: a plain C++ compiler can take this file.
#pragma once
#include <stdint.h>

#include "knn_args.hpp"

namespace wv {

constexpr int kIpMapMaxRows = WV_IP_MAP_ROWS_MAX;   // the ranked list of a query is sorted in one workgroup's LDS
constexpr int kIpMapMaxD = 512;                      // the query row staged in LDS, zero-padded to whole tiles of k

// wv_ip_map_at_k[_cpu].  what: the entry point's name in the message
inline int ip_map_args(const char *what, const void *q, const void *db, int Q, int64_t N, int D, const void *qlab,
                       const void *dblab, int lwords, int k, const void *ap)
{
    if (!q) WV_FAIL(WV_EINVAL, "%s: q is null", what);
    if (!db) WV_FAIL(WV_EINVAL, "%s: db is null", what);
    if (!qlab) WV_FAIL(WV_EINVAL, "%s: qlab is null", what);
    if (!dblab) WV_FAIL(WV_EINVAL, "%s: dblab is null", what);
    if (!ap) WV_FAIL(WV_EINVAL, "%s: ap is null", what);
    if (Q < 0) WV_FAIL(WV_EINVAL, "%s: Q=%d must be >= 0", what, Q);
    if (N < 1) WV_FAIL(WV_EINVAL, "%s: N=%lld must be >= 1", what, (long long)N);
    if (D < 1) WV_FAIL(WV_EINVAL, "%s: D=%d must be >= 1", what, D);
    if (!(k >= 1 && k <= N)) WV_FAIL(WV_EINVAL, "%s: k=%d must be in [1, N=%lld]", what, k, (long long)N);
    if (!(lwords == 1 || lwords == 2)) WV_FAIL(WV_EINVAL, "%s: lwords=%d (supported: 1, 2)", what, lwords);
    if (N > kIpMapMaxRows)
        WV_FAIL(WV_ENOTSUP, "%s: N=%lld above WV_IP_MAP_ROWS_MAX=%d rows (rank with wv_knn_float, then wv_map_at_k)", what,
                (long long)N, kIpMapMaxRows);
    if (D > kIpMapMaxD)
        WV_FAIL(WV_ENOTSUP, "%s: D=%d above the supported %d (rank with wv_knn_float, then wv_map_at_k)", what, D, kIpMapMaxD);
    return WV_OK;
}

}  // namespace wv
