// Host twin of wv_ip_map_at_k (ip_map.hip): the batch mAP proxy of real-valued embeddings on HOST pointers, for
// CustomCalculator(device='cpu', soft_codes=True).
//
// The contract defines the result as wv_map_at_k applied to the list wv_knn_float(metric IP, k) returns, so the twin IS that
// composition of the two existing twins, query block by query block: wv_knn_float_cpu forms every score as one fmaf chain in
// accumulation_order(D) (host_knn.cpp) and ranks on (order-preserving key, row); wv_map_at_k_cpu walks the list with
// wv_map_at_k's arithmetic and summation order (host_rank.cpp).  What this file adds is the entry point's own argument rules
// (ip_map.hpp, shared with the kernel) and the block loop that keeps the list at kBlock rows.  The kernel restates both
// stages on the device (scalar fmaf chains, an in-LDS sort, the walk of ap_walk.hpp); the GPU tests hold it to these bits.
// No HIP call, no thread, no global state.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ip_map.hpp"

namespace {
constexpr int kBlock = 64;    // queries ranked per call of the k-NN twin: the list stays at kBlock * k entries
}

extern "C" int wv_ip_map_at_k_cpu(const float *q, const float *db, int Q, int64_t N, int D, const uint64_t *qlab,
                                  const uint64_t *dblab, int lwords, int k, float *ap, int32_t *nrel)
{
    const int refused = wv::ip_map_args("ip_map_at_k_cpu", q, db, Q, N, D, qlab, dblab, lwords, k, ap);
    if (refused != WV_OK || Q == 0) return refused;
    std::vector<int32_t> idx((size_t)std::min(Q, kBlock) * k);
    std::vector<float> val(idx.size());
    for (int q0 = 0; q0 < Q; q0 += kBlock) {
        const int qc = std::min(kBlock, Q - q0);
        int rc = wv_knn_float_cpu(q + (size_t)q0 * D, db, qc, N, D, WV_METRIC_IP, k, idx.data(), val.data());
        if (rc != WV_OK) return rc;
        rc = wv_map_at_k_cpu(idx.data(), k, qc, k, qlab + (size_t)q0 * lwords, dblab, lwords, ap + q0, nrel ? nrel + q0 : nullptr);
        if (rc != WV_OK) return rc;
    }
    return WV_OK;
}
