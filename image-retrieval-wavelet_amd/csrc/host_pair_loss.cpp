// Host twin of wv_pair_loss (pair_loss.hip): SCHLoss / HashNetLoss, value and gradient w.r.t. the embeddings, on HOST
// pointers.  The argument rules, the per-pair term and the finishing scalars are pair_loss.hpp's, shared with the kernel;
// what this file adds is the plain double loop over the pairs.  fp32 throughout (G and the gradient sums are fmaf chains in
// index order), the two global sums in double as in the kernel.  The kernel groups its sums differently and the device's
// tanhf / expf / log1pf are not the host's: the two agree to fp32 rounding, not bit for bit.
// No HIP call, no thread, no global state.
#include <stdint.h>

#include <vector>

#include "pair_loss.hpp"

extern "C" int wv_pair_loss_cpu(const float *e, const uint64_t *labels, int lwords, int B, int D,
                                const wv_pair_loss_params *params, float *out, float *grad)
{
    const int refused = wv::pair_loss_args("pair_loss_cpu", e, labels, lwords, B, D, params, out, false, nullptr, 0);
    if (refused != WV_OK) return refused;
    const wv_pair_loss_params p = *params;
    const size_t n = (size_t)B * D;
    std::vector<float> u(n), g(grad ? 2 * n : 0, 0.f);
    std::vector<int> cnt(B);
    for (size_t x = 0; x < n; ++x) u[x] = wv::pl_squash(p, e[x]);
    auto word = [&](int i, int w) { return w < lwords ? labels[(size_t)i * lwords + w] : 0ull; };
    for (int i = 0; i < B; ++i) cnt[i] = wv::pl_popc(word(i, 0)) + wv::pl_popc(word(i, 1));
    double s1 = 0., s2 = 0.;
    uint64_t n1 = 0;
    for (int i = 0; i < B; ++i) {
        const float *ui = u.data() + (size_t)i * D;
        for (int j = 0; j < B; ++j) {
            const float *uj = u.data() + (size_t)j * D;
            float G = 0.f;
            for (int k = 0; k < D; ++k) G = fmaf(ui[k], uj[k], G);
            const int c = wv::pl_popc(word(i, 0) & word(j, 0)) + wv::pl_popc(word(i, 1) & word(j, 1));
            const wv::PairTerm t = wv::pair_term(p, G, cnt[i], cnt[j], c);
            s1 += t.v1, s2 += t.v2, n1 += (uint64_t)t.pos;
            if (grad) {
                float *g1 = g.data() + (size_t)i * D, *g2 = g1 + n;
                for (int k = 0; k < D; ++k) g1[k] = fmaf(t.a1, uj[k], g1[k]), g2[k] = fmaf(t.a2, uj[k], g2[k]);
            }
        }
    }
    const wv::PairLossScalars sc = wv::pair_loss_scalars(p, B, s1, s2, n1);
    out[0] = sc.loss, out[1] = sc.part1, out[2] = sc.part2;
    if (grad)
        for (size_t x = 0; x < n; ++x) grad[x] = fmaf(sc.kappa1, g[x], sc.kappa2 * g[n + x]) * wv::pl_chain(p, u[x]);
    return WV_OK;
}
