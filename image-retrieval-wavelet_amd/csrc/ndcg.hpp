// What the NDCG kernels (ndcg.hip) and their host twins (host_ndcg.cpp) share: the gain of a label overlap and the argument
// rules of the entry points.  Plain C++ (host_ndcg.cpp is compiled without the HIP headers); ndcg.hip includes common.hpp first.
#pragma once
#include <stdint.h>

#include "twin.hpp"

namespace wv {

// gain(r) = 2^r - 1 as an fp64 value, ldexp(1.0, r) - 1.0 built from the exponent field (0 <= r <= 128): exact through
// r = 53, the nearest double above (2^r from r = 54).  No transcendental, the same bits on the host and on the device.
WV_HD double ndcg_gain(int r)
{
    const uint64_t bits = (uint64_t)(1023 + r) << 52;
    double v;
    __builtin_memcpy(&v, &bits, sizeof v);
    return v - 1.0;
}

// wv_label_overlap_hist[_cpu]: answered before any pointer is read
inline int ndcg_hist_args(const char *what, bool buffers, int lwords, int Q, int64_t N)
{
    if (!buffers) WV_FAIL(WV_EINVAL, "%s: null buffer", what);
    if (lwords != 1 && lwords != 2) WV_FAIL(WV_ENOTSUP, "%s: lwords=%d (supported: 1, 2 -- up to 128 classes)", what, lwords);
    if (!(Q >= 0 && N >= 1 && N <= 0xffffffffLL)) WV_FAIL(WV_EINVAL, "%s: bad shape Q=%d N=%lld", what, Q, (long long)N);
    return WV_OK;
}

// wv_ndcg_at_ks[_cpu]: wv_map_at_ks' rules for the cut-offs (ks: HOST pointer, the only one read here)
inline int ndcg_walk_args(const char *what, bool buffers, int64_t ld, int Q, const int *ks, int nk, int lwords)
{
    if (!buffers) WV_FAIL(WV_EINVAL, "%s: null buffer", what);
    if (lwords != 1 && lwords != 2) WV_FAIL(WV_ENOTSUP, "%s: lwords=%d (supported: 1, 2 -- up to 128 classes)", what, lwords);
    if (!(Q >= 0 && ld >= 1)) WV_FAIL(WV_EINVAL, "%s: bad shape Q=%d ld=%lld", what, Q, (long long)ld);
    if (!ks) WV_FAIL(WV_EINVAL, "%s: null cut-off list", what);
    if (!(nk >= 1 && nk <= WV_MAX_CUTOFFS)) WV_FAIL(WV_EINVAL, "%s: %d cut-offs (supported: 1..%d)", what, nk, WV_MAX_CUTOFFS);
    if (ks[0] < 1) WV_FAIL(WV_EINVAL, "%s: cut-off %d must be >= 1", what, ks[0]);
    for (int i = 1; i < nk; ++i)
        if (ks[i] <= ks[i - 1])
            WV_FAIL(WV_EINVAL, "%s: cut-offs must be strictly ascending (ks[%d]=%d after %d)", what, i, ks[i], ks[i - 1]);
    if (ks[nk - 1] > ld) WV_FAIL(WV_EINVAL, "%s: largest cut-off %d must be <= ld=%lld", what, ks[nk - 1], (long long)ld);
    return WV_OK;
}

}  // namespace wv
