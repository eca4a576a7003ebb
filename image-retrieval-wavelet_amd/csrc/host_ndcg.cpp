// Host twins of the NDCG entry points (ndcg.hip) and the weight table both sides read.  HOST pointers, no HIP call, no thread,
// no global state.  The overlap histogram is integers; DCG and ideal DCG are the kernel's bits: the same gains (ndcg.hpp), the
// same table w, an explicit fma per term in increasing position on the accumulator of thread p % 256, every cut-off reduced
// in the kernel's order (lanes in wave_sum_f64's butterfly, the four waves in index order).  Compiled without contraction.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ndcg.hpp"

using namespace wv;

namespace {

// the 256 threads' sums in k_ndcg_at_ks' order
inline double sum_in_kernel_order(const double (&acc)[256])
{
    double wave[4];
    for (int w = 0; w < 4; ++w) {                                           // wave_sum_f64: v += shfl_xor(v, d), d = 32 .. 1
        double s[64];
        for (int l = 0; l < 64; ++l) s[l] = acc[64 * w + l];
        for (int dd = 32; dd > 0; dd >>= 1) {
            double n2[64];
            for (int l = 0; l < 64; ++l) n2[l] = s[l] + s[l ^ dd];
            for (int l = 0; l < 64; ++l) s[l] = n2[l];
        }
        wave[w] = s[0];
    }
    return wave[0] + wave[1] + wave[2] + wave[3];
}

inline int overlap(const uint64_t *ql, const uint64_t *dl, int lwords)
{
    int r = 0;
    for (int w = 0; w < lwords; ++w) r += __builtin_popcountll(ql[w] & dl[w]);
    return r;
}

}  // namespace

// w[p] = 1 / log2(p + 2): the only logarithm and the only division of the metric, made once
extern "C" int wv_ndcg_weights(double *w, int64_t k)
{
    if (!w) WV_FAIL(WV_EINVAL, "ndcg_weights: null buffer");
    if (k < 0) WV_FAIL(WV_EINVAL, "ndcg_weights: k=%lld", (long long)k);
    for (int64_t p = 0; p < k; ++p) w[p] = 1.0 / log2((double)(p + 2));
    return WV_OK;
}

extern "C" int wv_label_overlap_hist_cpu(const uint64_t *qlab, const uint64_t *dblab, int lwords, int Q, int64_t N, uint32_t *hist)
{
    if (int rc = ndcg_hist_args("label_overlap_hist_cpu", qlab && dblab && hist, lwords, Q, N)) return rc;
    const int bins = 64 * lwords + 1;
    for (int qi = 0; qi < Q; ++qi) {
        const uint64_t *ql = qlab + (int64_t)qi * lwords;
        uint32_t *h = hist + (int64_t)qi * bins;
        memset(h, 0, sizeof(uint32_t) * (size_t)bins);
        for (int64_t n = 0; n < N; ++n) h[overlap(ql, dblab + n * lwords, lwords)]++;
    }
    return WV_OK;
}

extern "C" int wv_ndcg_at_ks_cpu(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab,
                                 const uint64_t *dblab, int lwords, const uint32_t *hist, const double *w, double *dcg, double *idcg)
{
    if (int rc = ndcg_walk_args("ndcg_at_ks_cpu", idx && qlab && dblab && hist && w && dcg && idcg, ld, Q, ks, nk, lwords)) return rc;
    const int B = 64 * lwords, bins = B + 1;
    for (int qi = 0; qi < Q; ++qi) {
        const int32_t *list = idx + (int64_t)qi * ld;
        const uint64_t *ql = qlab + (int64_t)qi * lwords;
        const uint32_t *h = hist + (int64_t)qi * bins;
        double accd[256], acci[256];
        for (int t = 0; t < 256; ++t) accd[t] = acci[t] = 0.0;
        // ideal list: the gains of all rows, descending -- position p takes the largest r with #{rel >= r} > p
        int best = B;
        uint64_t ge = h[B];                                                 // rows with rel >= best
        int next = 0;
        for (int p = 0; p < ks[nk - 1]; ++p) {
            const int32_t id = list[p];
            const int rel = id >= 0 ? overlap(ql, dblab + (int64_t)id * lwords, lwords) : 0;
            while (best >= 1 && ge <= (uint64_t)p) ge += h[--best];        // best = 0: past the last row with rel >= 1
            accd[p & 255] = fma(ndcg_gain(rel), w[p], accd[p & 255]);
            acci[p & 255] = fma(ndcg_gain(best), w[p], acci[p & 255]);
            if (p + 1 == ks[next]) {
                dcg[(int64_t)qi * nk + next] = sum_in_kernel_order(accd);
                idcg[(int64_t)qi * nk + next] = sum_in_kernel_order(acci);
                ++next;
            }
        }
    }
    return WV_OK;
}
