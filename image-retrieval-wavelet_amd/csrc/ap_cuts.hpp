// The cut-offs of an average-precision call at several cut-offs, and THE rule for them: what the walk (ap_walk.hpp), the entry
// points that launch it (topk.hip, merge.hip, list_ap.hip) and the host twin (host_rank.cpp) share.  No HIP header is
// included, so a plain C++ compiler can take this file.
#pragma once
#include <stdint.h>

#include "twin.hpp"

namespace wv {

constexpr int kMaxCutoffs = 16;
static_assert(kMaxCutoffs == WV_MAX_CUTOFFS, "ap_cuts.hpp and wvhash.h disagree");

struct ApCuts {                              // travels by value in the kernel arguments: no device copy, no sync
    int n;                                   // 1 .. kMaxCutoffs
    int k[kMaxCutoffs];                      // strictly ascending, k[0] >= 1; the walk is k[n - 1] positions long
};

// The cut-offs of a call (HOST pointer): 1 .. WV_MAX_CUTOFFS of them, strictly ascending, inside [1, limit].
inline int validate_cuts(const char *what, const int *ks, int nk, int64_t limit, const char *limit_name, ApCuts &cuts)
{
    WV_REQUIRE(ks, "%s: null cut-off list", what);
    WV_REQUIRE(nk >= 1 && nk <= kMaxCutoffs, "%s: %d cut-offs (supported: 1..%d)", what, nk, kMaxCutoffs);
    cuts.n = nk;
    for (int i = 0; i < kMaxCutoffs; ++i) cuts.k[i] = i < nk ? ks[i] : 0;
    WV_REQUIRE(ks[0] >= 1, "%s: cut-off %d must be >= 1", what, ks[0]);
    for (int i = 1; i < nk; ++i)
        WV_REQUIRE(ks[i] > ks[i - 1], "%s: cut-offs must be strictly ascending (ks[%d]=%d after %d)", what, i, ks[i], ks[i - 1]);
    WV_REQUIRE(ks[nk - 1] <= limit, "%s: largest cut-off %d must be <= %s=%lld", what, ks[nk - 1], limit_name, (long long)limit);
    return WV_OK;
}

}  // namespace wv
