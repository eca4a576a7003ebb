// Host twin of wv_knn_float ("wv_l2_topk / wv_ip_topk ... _cpu twins of each taking host pointers"):
// get_knn_torch's cosine / l2 branches (/root/reference/main/engine/get_knn.py:60-71) and the faiss IndexFlatL2 flavour
// (:38-39,55) on HOST pointers, for CustomCalculator(device='cpu') with real-valued embeddings.
//
// Same results as the gfx950 path, bit for bit:
//  * v_mfma_f32_32x32x2_f32 IS an fmaf chain -- D = fma(a1, b1, fma(a0, b0, C)), k = 0 before k = 1, every one of 204,800
//    random outputs (tools/mfma_order_test.hip) -- and k_scores_lds feeds it k = 8c + e (lane half 0) and 8c + 4 + e (half 1)
//    for e = 0..3 of every chunk c of eight; the zero padding beyond D adds exact zeros.  The dot product below walks k in
//    that order with fused multiply-adds (the FMA instruction when the CPU has it, fmaf otherwise: the same bits);
//  * |x|^2 as k_row_sqnorm forms it: lane l of a wave sums k = l, l + 64, ... with fmaf, the 64 partial sums meet in the
//    xor butterfly 32, 16, ..., 1;  d2 = max(0, fma(-2, q.r, |q|^2 + |r|^2)), ranked squared, the root taken of the k results;
//  * ranking: ascending (order-preserving key of the score, database row) -- what both GPU rankings produce.
// No HIP call, no thread, no global state.  Product code: shares nothing with oracle/.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "knn_args.hpp"

namespace {

constexpr int kLanes = 8;     // database rows per vector
constexpr int kBlocks = 8;    // vectors in flight per query: eight independent fma chains

using wv::float_to_key;
using wv::key_to_float;

// k in the order the matrix cores accumulate it
std::vector<int> accumulation_order(int D)
{
    std::vector<int> ord;
    ord.reserve(D);
    for (int c = 0; 8 * c < D; ++c)
        for (int e = 0; e < 4; ++e) {
            if (8 * c + e < D) ord.push_back(8 * c + e);
            if (8 * c + 4 + e < D) ord.push_back(8 * c + 4 + e);
        }
    return ord;
}

float sqnorm_like_the_kernel(const float *x, int D)
{
    float s[64];
    for (int l = 0; l < 64; ++l) {
        float a = 0.f;
        for (int k = l; k < D; k += 64) a = fmaf(x[k], x[k], a);
        s[l] = a;
    }
    for (int d = 32; d > 0; d >>= 1) {
        float t[64];
        for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ d];
        memcpy(s, t, sizeof(s));
    }
    return s[0];
}

// scores of one query against kBlocks * kLanes database rows of the interleaved image bt[block][j][lane]
void dots_plain(const float *qo, const float *bt, int D, float *out)
{
    for (int b = 0; b < kBlocks; ++b)
        for (int l = 0; l < kLanes; ++l) {
            float acc = 0.f;
            const float *col = bt + (size_t)b * D * kLanes + l;
            for (int j = 0; j < D; ++j) acc = fmaf(qo[j], col[(size_t)j * kLanes], acc);
            out[b * kLanes + l] = acc;
        }
}
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) void dots_fma(const float *qo, const float *bt, int D, float *out)
{
    __m256 acc[kBlocks];
    for (int b = 0; b < kBlocks; ++b) acc[b] = _mm256_setzero_ps();
    const size_t pitch = (size_t)D * kLanes;
    for (int j = 0; j < D; ++j) {
        const __m256 a = _mm256_broadcast_ss(qo + j);
        const float *p = bt + (size_t)j * kLanes;
        for (int b = 0; b < kBlocks; ++b) acc[b] = _mm256_fmadd_ps(a, _mm256_loadu_ps(p + b * pitch), acc[b]);
    }
    for (int b = 0; b < kBlocks; ++b) _mm256_storeu_ps(out + b * kLanes, acc[b]);
}
#endif
void dots(const float *qo, const float *bt, int D, float *out)
{
#if defined(__x86_64__)
    static const int has = (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) ? 1 : 0;
    if (has) return dots_fma(qo, bt, D, out);
#endif
    dots_plain(qo, bt, D, out);
}

// The closing step of both twins: the k best of a row's (key << 32 | column) words in ascending order -> index and value lists
void rank_and_write(std::vector<uint64_t> &keyed, int k, bool desc, bool root, int32_t *idx, float *val)
{
    if ((size_t)k < keyed.size()) std::nth_element(keyed.begin(), keyed.begin() + k, keyed.end());
    std::sort(keyed.begin(), keyed.begin() + k);
    for (int j = 0; j < k; ++j) {
        const uint64_t e = keyed[(size_t)j];
        const float v = key_to_float((uint32_t)(e >> 32), desc);
        idx[j] = (int32_t)(uint32_t)e;
        val[j] = root ? sqrtf(v) : v;
    }
}

}  // namespace

extern "C" int wv_knn_float_cpu(const float *q, const float *db, int Q, int64_t N, int D, int metric, int k, int32_t *idx,
                                float *val)
{
    const int refused = wv::knn_float_args("knn_float_cpu", q && db && idx && val, Q, N, D, metric, k);
    if (refused != WV_OK || Q == 0) return refused;
    const bool l2 = metric != WV_METRIC_IP, desc = !l2;
    const std::vector<int> ord = accumulation_order(D);
    // database rows interleaved eight by eight, k in accumulation order (rows beyond N are zeros and never ranked)
    const int64_t group = (int64_t)kBlocks * kLanes, Np = (N + group - 1) / group * group;
    std::vector<float> bt((size_t)Np * D, 0.f);
    for (int64_t n = 0; n < N; ++n) {
        float *dst = bt.data() + (size_t)(n / kLanes) * D * kLanes + n % kLanes;
        const float *src = db + (size_t)n * D;
        for (int j = 0; j < D; ++j) dst[(size_t)j * kLanes] = src[ord[j]];
    }
    std::vector<float> dbn;
    if (l2) {
        dbn.resize((size_t)N);
        for (int64_t n = 0; n < N; ++n) dbn[(size_t)n] = sqnorm_like_the_kernel(db + (size_t)n * D, D);
    }
    std::vector<float> qo((size_t)D), row((size_t)Np);
    std::vector<uint64_t> keyed((size_t)N);
    for (int qi = 0; qi < Q; ++qi) {
        const float *qr = q + (size_t)qi * D;
        for (int j = 0; j < D; ++j) qo[(size_t)j] = qr[ord[j]];
        for (int64_t n0 = 0; n0 < Np; n0 += group) dots(qo.data(), bt.data() + (size_t)n0 * D, D, row.data() + n0);
        const float qn = l2 ? sqnorm_like_the_kernel(qr, D) : 0.f;
        for (int64_t n = 0; n < N; ++n) {
            float v = row[(size_t)n];
            if (l2) v = fmaxf(0.f, fmaf(-2.f, v, qn + dbn[(size_t)n]));
            keyed[(size_t)n] = ((uint64_t)float_to_key(v, desc) << 32) | (uint32_t)n;
        }
        rank_and_write(keyed, k, desc, metric == WV_METRIC_L2, idx + (size_t)qi * k, val + (size_t)qi * k);
    }
    return WV_OK;
}

extern "C" int wv_rank_scores_cpu(const float *S, int Q, int64_t N, int k, int flags, int32_t *idx, float *val)
{
    const int refused = wv::rank_scores_args("rank_scores_cpu", S && idx && val, Q, N, k, flags);
    if (refused != WV_OK) return refused;
    const bool desc = (flags & WV_RANK_DESCENDING) != 0, root = (flags & WV_RANK_SQRT) != 0;
    std::vector<uint64_t> keyed((size_t)N);
    for (int qi = 0; qi < Q; ++qi) {
        const float *row = S + (size_t)qi * N;
        for (int64_t n = 0; n < N; ++n) keyed[(size_t)n] = ((uint64_t)float_to_key(row[n], desc) << 32) | (uint32_t)n;
        rank_and_write(keyed, k, desc, root, idx + (size_t)qi * k, val + (size_t)qi * k);
    }
    return WV_OK;
}
