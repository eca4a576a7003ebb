// Host twin of wv_rank_ap (rank_ap.hip): SmoothAP / SupAP, AP per query row and its gradient w.r.t. the row's scores, on
// HOST pointers.  The argument rules, the per-pair term, the positive's record and the gradient coefficient are
// rank_ap.hpp's, shared with the kernel; what this file adds is the bit rows and the plain loops over rows, positives and
// columns.  The pair terms are fp32 as in the kernel; the sums over the columns and over the positives are kept in double
// (the kernel adds 64 fp32 lane sums by a tree, a serial fp32 sum of 4096 terms would be the looser of the two).  The
// device's expf is not the host's: the two agree to fp32 rounding, not bit for bit.
// No HIP call, no thread, no global state.
#include <stdint.h>

#include <vector>

#include "rank_ap.hpp"

extern "C" int wv_rank_ap_cpu(const float *scores, const float *target, int B, int M, const wv_rank_ap_params *params,
                              float *ap, float *grad)
{
    const int refused = wv::rank_ap_args("rank_ap_cpu", scores, target, B, M, params, ap, false, nullptr, 0);
    if (refused != WV_OK) return refused;
    const wv_rank_ap_params p = *params;
    const bool quick = p.form == WV_RANK_AP_QUICK;
    const int W = wv::rank_ap_words(M);
    std::vector<uint64_t> bits((size_t)B * W, 0), lm(quick ? (size_t)B * W : 0, 0);
    for (int q = 0; q < B; ++q)
        for (int j = 0; j < M; ++j)
            if (target[(size_t)q * M + j] != 0.f) bits[(size_t)q * W + j / 64] |= 1ull << (j % 64);
    if (quick)
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < B; ++j) {
                bool hit = false;
                for (int w = 0; w < W && !hit; ++w) hit = (bits[(size_t)i * W + w] & bits[(size_t)j * W + w]) != 0;
                if (hit) lm[(size_t)i * W + j / 64] |= 1ull << (j % 64);
            }
    auto bit = [&](const std::vector<uint64_t> &rows, int r, int j) { return (rows[(size_t)r * W + j / 64] >> (j % 64)) & 1; };

    std::vector<int> pos;
    std::vector<double> g(M);
    for (int q = 0; q < B; ++q) {
        const float *S = scores + (size_t)q * M;
        pos.clear();
        for (int j = 0; j < M; ++j)
            if (bit(bits, q, j)) pos.push_back(j);
        const int np = (int)pos.size();
        std::fill(g.begin(), g.end(), 0.);
        double sum_f = 0.;
        for (int i : pos) {
            auto w_of = [&](int j) { return quick ? bit(bits, i, j) != 0 : bit(bits, q, j) != 0; };
            auto tgt_of = [&](int j) { return quick ? (bit(lm, i, j) & bit(bits, q, j)) != 0 : bit(bits, q, j) != 0; };
            double sR = 0., sRw = 0., sD = 0., sDw = 0.;
            for (int j = 0; j < M; ++j) {
                if (j == i) continue;
                const wv::RankTerm r = wv::rank_term(p, S[j] - S[i], tgt_of(j));
                const bool w = w_of(j);
                sR += r.R, sRw += w ? r.R : 0.f;
                sD += r.dR, sDw += w ? r.dR : 0.f;
            }
            const wv::RankApRecord rec = wv::rank_ap_record((float)sR, (float)sRw, (float)sD, (float)sDw, np);
            sum_f += rec.f;
            if (grad) {
                for (int j = 0; j < M; ++j) {
                    if (j == i) continue;
                    const wv::RankTerm r = wv::rank_term(p, S[j] - S[i], tgt_of(j));
                    g[j] += wv::rank_ap_coeff(rec, w_of(j), r.dR);
                }
                g[i] -= rec.own;
            }
        }
        ap[q] = np > 0 ? (float)(sum_f / np) : 0.f;
        if (grad)
            for (int j = 0; j < M; ++j) grad[(size_t)q * M + j] = (float)g[j];
    }
    return WV_OK;
}
