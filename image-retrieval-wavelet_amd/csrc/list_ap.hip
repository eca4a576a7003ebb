// Metrics over written ranked lists for gfx950: average precision at one cut-off (k_map_at_k) or at several (k_map_at_ks),
// and running hit counts (k_hit_prefix).  One workgroup (256 threads) takes one query's list.
//
// AP over a ranked list (accuracy_calculator.py:222-229): hits at 1-based ranks r_1 < r_2 < ...
// give AP = mean_j (j / r_j); relevance = labels share a bit (label_comparison_fn :31-37).
#include <type_traits>

#include "ap_walk.hpp"

namespace wv {

// Does a list entry share a label bit with query qi?  LW = 1, 2: that many label words, the query's kept in registers;
// LW = 0: any number (lwords), read in the loop.  An absent entry (< 0) reads row 0 and counts as no hit.
template <int LW>
struct ListRelevance {
    const uint64_t *dblab, *ql;
    int lwords;
    uint64_t qreg[LW > 0 ? LW : 1];
    __device__ __forceinline__ ListRelevance(const uint64_t *qlab, const uint64_t *dblab_, int lwords_, int qi)
        : dblab(dblab_), lwords(lwords_)
    {
        ql = qlab + (int64_t)qi * (LW > 0 ? LW : lwords);
        if constexpr (LW > 0) {
#pragma unroll
            for (int w = 0; w < LW; ++w) qreg[w] = ql[w];
        }
    }
    __device__ __forceinline__ bool operator()(int32_t id) const
    {
        const int lw = LW > 0 ? LW : lwords;
        const uint64_t *dl = dblab + (int64_t)max(id, 0) * lw;
        uint64_t any = 0;
        if constexpr (LW > 0) {
#pragma unroll
            for (int w = 0; w < LW; ++w) any |= dl[w] & qreg[w];
        } else {
            for (int w = 0; w < lw; ++w) any |= dl[w] & ql[w];
        }
        return id >= 0 && any != 0;
    }
};

// AP of every query's list (row pitch ld) at one cut-off k.  k_map_at_ks below with one cut-off returns the same bits, but
// was measured 1 - 17 % slower at k = 5000 (profiles/list_ap_merge_refactor.txt), so wv_map_at_k[_ld] keep this kernel.
template <int LW>
__global__ __launch_bounds__(256) void k_map_at_k(const int32_t *__restrict__ idx, int64_t ld, int k,
                                                  const uint64_t *__restrict__ qlab,
                                                  const uint64_t *__restrict__ dblab, int lwords,
                                                  float *__restrict__ ap, int32_t *__restrict__ nrel)
{
    __shared__ uint32_t wave_cnt[4];
    __shared__ double wave_sum[4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int32_t *list = idx + (int64_t)qi * ld;
    const ListRelevance<LW> relevant(qlab, dblab, lwords, qi);
    uint32_t running = 0;
    double acc = 0.0;
    for (int p0 = 0; p0 < k; p0 += 256) {
        const int p = p0 + tid;
        const bool rel = p < k && relevant(list[p]);
        const uint64_t mask = __ballot(rel);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = running;
        for (int w2 = 0; w2 < wv; ++w2) before += wave_cnt[w2];
        const uint32_t block_total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (rel) {
            const uint32_t j = before + (uint32_t)mbcnt(mask) + 1;  // this is the j-th hit
            acc += (double)((float)j / (float)(p + 1));             // fp32 quotient like the reference
        }
        running += block_total;
        __syncthreads();
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) wave_sum[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        const double s = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        ap[qi] = running ? (float)(s / (double)running) : 0.0f;
        if (nrel) nrel[qi] = (int32_t)running;
    }
}

// The same at the cut-offs `cuts` (wv_map_at_ks): the list is read and the labels are gathered once, ap / nrel are
// [Q][cuts.n].  The walk is ap_walk.hpp's: the column of cut-off c has the bits of k_map_at_k at k = c.
template <int LW>
__global__ __launch_bounds__(256) void k_map_at_ks(const int32_t *__restrict__ idx, int64_t ld, const uint64_t *__restrict__ qlab,
                                                   const uint64_t *__restrict__ dblab, int lwords, float *__restrict__ ap,
                                                   int32_t *__restrict__ nrel, ApCuts cuts)
{
    __shared__ __attribute__((aligned(8))) uint32_t scratch[ap_cuts_scratch_dwords<256>()];
    const int qi = blockIdx.x, k = cuts.k[cuts.n - 1];
    const int32_t *list = idx + (int64_t)qi * ld;
    const ListRelevance<LW> relevant(qlab, dblab, lwords, qi);
    walk_cuts_256([&](int p) { return relevant(list[p]); }, k, scratch, cuts, ap + (int64_t)qi * cuts.n,
                  nrel ? nrel + (int64_t)qi * cuts.n : nullptr);
}

// Running hit count along a ranked list: hits[q][p] = number of relevant entries among list[0..p]
// (relevance as in k_map_at_ks).  Precision@p, recall@p, R-precision and the precision/recall curves of
// accuracy_calculator.py:131-181,235-273 are ratios of these counts.
// As in the AP kernels, an absent entry (< 0) reads label row 0 and counts as no hit: no load is skipped.
__global__ __launch_bounds__(256) void k_hit_prefix(const int32_t *__restrict__ idx, int k,
                                                    const uint64_t *__restrict__ qlab,
                                                    const uint64_t *__restrict__ dblab, int lwords,
                                                    uint32_t *__restrict__ hits)
{
    __shared__ uint32_t wave_cnt[4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int32_t *list = idx + (int64_t)qi * k;
    const ListRelevance<0> relevant(qlab, dblab, lwords, qi);
    uint32_t running = 0;
    for (int p0 = 0; p0 < k; p0 += 256) {
        const int p = p0 + tid;
        const bool rel = p < k && relevant(list[p]);
        const uint64_t mask = __ballot(rel);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = running;
        for (int w2 = 0; w2 < wv; ++w2) before += wave_cnt[w2];
        if (p < k) hits[(int64_t)qi * k + p] = before + (uint32_t)mbcnt(mask) + (rel ? 1u : 0u);
        running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
}

// THE dispatch on the number of label words: launch(LW) with LW = 1, 2 or 0 (the generic loop) as a compile-time constant
template <typename LAUNCH>
static void by_label_words(int lwords, LAUNCH launch)
{
    if (lwords == 1) launch(std::integral_constant<int, 1>{});
    else if (lwords == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 0>{});
}

}  // namespace wv

using namespace wv;

extern "C" int wv_map_at_k_ld(const int32_t *idx, int64_t ld, int Q, int k, const uint64_t *qlab,
                              const uint64_t *dblab, int lwords, float *ap, int32_t *nrel, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && ap, "map_at_k: null buffer");
    WV_REQUIRE(Q >= 0 && k >= 1 && lwords >= 1 && ld >= k, "map_at_k: bad shape Q=%d k=%d ld=%lld lwords=%d", Q, k, (long long)ld, lwords);
    if (Q == 0) return WV_OK;
    by_label_words(lwords, [&](auto lw) {
        hipLaunchKernelGGL((k_map_at_k<lw()>), dim3(Q), dim3(256), 0, (hipStream_t)stream, idx, ld, k, qlab, dblab, lwords, ap, nrel);
    });
    WV_CHECK_LAUNCH("k_map_at_k");
    return WV_OK;
}

extern "C" int wv_map_at_k(const int32_t *idx, int Q, int k, const uint64_t *qlab,
                           const uint64_t *dblab, int lwords, float *ap, int32_t *nrel, void *stream)
{
    return wv_map_at_k_ld(idx, k, Q, k, qlab, dblab, lwords, ap, nrel, stream);
}

extern "C" int wv_map_at_ks(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                            int lwords, float *ap, int32_t *nrel, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && ap, "map_at_ks: null buffer");
    WV_REQUIRE(Q >= 0 && lwords >= 1 && ld >= 1, "map_at_ks: bad shape Q=%d ld=%lld lwords=%d", Q, (long long)ld, lwords);
    ApCuts cuts;
    if (int rc = validate_cuts("map_at_ks", ks, nk, ld, "ld", cuts)) return rc;
    if (Q == 0) return WV_OK;
    by_label_words(lwords, [&](auto lw) {
        hipLaunchKernelGGL((k_map_at_ks<lw()>), dim3(Q), dim3(256), 0, (hipStream_t)stream, idx, ld, qlab, dblab, lwords, ap, nrel, cuts);
    });
    WV_CHECK_LAUNCH("k_map_at_ks");
    return WV_OK;
}

extern "C" int wv_hit_prefix(const int32_t *idx, int Q, int k, const uint64_t *qlab, const uint64_t *dblab,
                             int lwords, uint32_t *hits, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && hits, "hit_prefix: null buffer");
    WV_REQUIRE(Q >= 0 && k >= 1 && lwords >= 1, "hit_prefix: bad shape Q=%d k=%d lwords=%d", Q, k, lwords);
    if (Q == 0) return WV_OK;
    hipLaunchKernelGGL(k_hit_prefix, dim3(Q), dim3(256), 0, (hipStream_t)stream, idx, k, qlab, dblab, lwords, hits);
    WV_CHECK_LAUNCH("k_hit_prefix");
    return WV_OK;
}
