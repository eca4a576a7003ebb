// What wv_pair_loss (pair_loss.hip) and its host twin (host_pair_loss.cpp) share: the limits, the argument rules -- every
// refusal is answered here, before any pointer is read and before any HIP call --, the workspace layout, the per-pair term
// of both losses and the two scalars the finishing step forms.  No HIP header is included: a plain C++ compiler can take
// this file.
//
// Both losses are  f(G, R)  of the Gram matrix G = u u^T of the (tanh'ed) batch and a relation R read from the packed
// multi-hot labels.  A pair (i, j) yields two values v1, v2 whose sums over all B^2 pairs make the two parts of the loss,
// and two coefficients a1, a2: the gradient of part p w.r.t. u_i is  kappa_p * sum_j a_p(i, j) u_j  (f is symmetric in
// (i, j), so a row owner has the whole sum), kappa_p a function of the global sums alone.
//   SCH      (main/losses/dsch.py:31-59)           v_p = r_p^2, a_p = r_p W_p,  part_p = sqrt(sum v_p) / B^2
//   HashNet  (main/losses/hashnet_loss.py:49-66)   v = softplus(dp) - P dp, a = alpha (sigmoid(dp) - P), split by P
#pragma once
#include <math.h>
#include <stdint.h>

#include "twin.hpp"

namespace wv {

constexpr int kPairLossMaxRows = WV_PAIR_LOSS_ROWS_MAX;
constexpr int kPairLossMaxD = 512;       // a row block and a column tile of u live in one workgroup's LDS
constexpr int kPlRows = 8;               // rows i a workgroup owns
constexpr int kPlCols = 32;              // columns j of one tile: kPlRows * kPlCols pairs = one per thread

// per-workgroup record of the main kernel, reduced in index order by the finishing step
struct PairLossPartial {
    double s1, s2;       // sums of v1, v2 over the workgroup's pairs
    uint64_t n1;         // HashNet: pairs that share a label
    uint64_t pad;
};

inline int pair_loss_blocks(int B) { return (B + kPlRows - 1) / kPlRows; }
inline size_t pair_loss_g_bytes(int B, int D) { return ((size_t)2 * B * D * sizeof(float) + 15) / 16 * 16; }
inline size_t pair_loss_ws_bytes(int B, int D)
{
    if (B < 1 || D < 1) return 0;
    return pair_loss_g_bytes(B, D) + (size_t)pair_loss_blocks(B) * sizeof(PairLossPartial);
}

// wv_pair_loss[_cpu].  what: the entry point's name in the message; device: the workspace is part of the call
inline int pair_loss_args(const char *what, const void *e, const void *labels, int lwords, int B, int D,
                          const wv_pair_loss_params *p, const void *out, bool device, const void *ws, size_t ws_bytes)
{
    if (!e) WV_FAIL(WV_EINVAL, "%s: e is null", what);
    if (!labels) WV_FAIL(WV_EINVAL, "%s: labels is null", what);
    if (!p) WV_FAIL(WV_EINVAL, "%s: params is null", what);
    if (!out) WV_FAIL(WV_EINVAL, "%s: out is null", what);
    if (B < 1) WV_FAIL(WV_EINVAL, "%s: B=%d must be >= 1", what, B);
    if (D < 1) WV_FAIL(WV_EINVAL, "%s: D=%d must be >= 1", what, D);
    if (!(lwords == 1 || lwords == 2)) WV_FAIL(WV_EINVAL, "%s: lwords=%d (supported: 1, 2)", what, lwords);
    if (!(p->kind == WV_PAIR_LOSS_SCH || p->kind == WV_PAIR_LOSS_HASHNET))
        WV_FAIL(WV_EINVAL, "%s: kind=%d (supported: WV_PAIR_LOSS_SCH, WV_PAIR_LOSS_HASHNET)", what, p->kind);
    if (!(p->pre_scale > 0.f)) WV_FAIL(WV_EINVAL, "%s: pre_scale=%g must be > 0", what, (double)p->pre_scale);
    if (B > kPairLossMaxRows)
        WV_FAIL(WV_ENOTSUP, "%s: B=%d above WV_PAIR_LOSS_ROWS_MAX=%d rows", what, B, kPairLossMaxRows);
    if (D > kPairLossMaxD) WV_FAIL(WV_ENOTSUP, "%s: D=%d above the supported %d", what, D, kPairLossMaxD);
    if (device) {
        if (!ws) WV_FAIL(WV_EINVAL, "%s: workspace is null", what);
        if (ws_bytes < pair_loss_ws_bytes(B, D))
            WV_FAIL(WV_EINVAL, "%s: workspace of %zu bytes, %zu needed (wv_pair_loss_workspace_bytes)", what, ws_bytes,
                    pair_loss_ws_bytes(B, D));
        if (reinterpret_cast<uintptr_t>(ws) & 15) WV_FAIL(WV_EINVAL, "%s: workspace must be 16-byte aligned", what);
    }
    return WV_OK;
}

WV_HD int pl_popc(uint64_t w) { return __builtin_popcountll(w); }

// u = tanh(pre_scale * e) or pre_scale * e, and d u / d e from u
WV_HD float pl_squash(const wv_pair_loss_params &p, float e)
{
    const float x = p.pre_scale * e;
    return p.apply_tanh ? tanhf(x) : x;
}
WV_HD float pl_chain(const wv_pair_loss_params &p, float u) { return p.apply_tanh ? p.pre_scale * (1.f - u * u) : p.pre_scale; }

struct PairTerm {
    float v1, v2;     // summed over all pairs
    float a1, a2;     // coefficient of u_j in the unnormalised gradient of part 1 / part 2 w.r.t. u_i
    int pos;          // HashNet: the pair shares a label
};

// One pair.  G: u_i . u_j;  ni, nj, c: |L_i|, |L_j|, |L_i & L_j|
WV_HD PairTerm pair_term(const wv_pair_loss_params &p, float G, int ni, int nj, int c)
{
    PairTerm t;
    if (p.kind == WV_PAIR_LOSS_SCH) {
        const float k = p.nbits;
        const bool same = c > 0 && c == ni && c == nj, disjoint = c == 0;
        // S = c / sqrt(ni nj): ni nj <= 128^2 is exact in fp32; `same` is decided on the integers, never on S == 1
        const float S = disjoint ? 0.f : (float)c / sqrtf((float)(ni * nj));
        const float lam = same ? 0.f : (1.f - S) * k * 0.5f;
        const float lam_l = disjoint ? k * 0.5f : fmaxf(lam - 3.f, 0.f);
        const float wl = same ? 0.f : (disjoint ? p.beta : 1.f);
        const float wu = same ? p.alpha : (disjoint ? 0.f : 1.f);
        const float H = (k - G) * 0.5f;
        const float r1 = fmaxf(lam_l - H, 0.f) * wl, r2 = fmaxf(H - lam, 0.f) * wu;
        t.v1 = r1 * r1, t.v2 = r2 * r2;
        t.a1 = r1 * wl, t.a2 = r2 * wu;
        t.pos = 0;
    } else {
        // softplus(dp) - P dp = softplus(-dp) for P, softplus(dp) otherwise; its derivative -sigmoid(-dp) | sigmoid(dp).
        // With x = -dp | dp: softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = (x >= 0 ? 1 : e) / (1 + e): no
        // difference of large numbers anywhere, so a saturated pair keeps its relative accuracy
        const bool P = c > 0;
        const float dp = p.alpha * G, x = P ? -dp : dp, e = expf(-fabsf(x));
        const float sp = fmaxf(x, 0.f) + log1pf(e);
        const float sg = (x >= 0.f ? 1.f : e) / (1.f + e);
        t.pos = P;
        t.v1 = P ? sp : 0.f, t.v2 = P ? 0.f : sp;
        t.a1 = P ? -p.alpha * sg : 0.f, t.a2 = P ? 0.f : p.alpha * sg;
    }
    return t;
}

struct PairLossScalars {
    float loss, part1, part2;
    float kappa1, kappa2;     // grad_i = (kappa1 g1_i + kappa2 g2_i) * chain
};

// The global sums -> the loss, its two parts and the factors of the two unnormalised gradient sums.  A part that is empty
// (HashNet: S1 or S0 = 0) or whose norm is 0 (SCH) contributes value 0 and gradient 0, as torch.norm's backward does.
WV_HD PairLossScalars pair_loss_scalars(const wv_pair_loss_params &p, int B, double s1, double s2, uint64_t n1)
{
    PairLossScalars r;
    const double BB = (double)B * (double)B;
    if (p.kind == WV_PAIR_LOSS_SCH) {
        const double q1 = sqrt(s1), q2 = sqrt(s2);
        r.part1 = (float)(q1 / BB), r.part2 = (float)(q2 / BB);
        r.kappa1 = q1 > 0. ? (float)(1. / (BB * q1)) : 0.f;          // 2 (symmetry) x 1/2 (H = (k - G) / 2) / (B^2 norm)
        r.kappa2 = q2 > 0. ? (float)(-1. / (BB * q2)) : 0.f;
    } else {
        const double S1 = (double)n1, S0 = BB - S1;
        r.part1 = S1 > 0. ? (float)(s1 / S1) : 0.f, r.part2 = S0 > 0. ? (float)(s2 / S0) : 0.f;
        r.kappa1 = S1 > 0. ? (float)(2. / S1) : 0.f;
        r.kappa2 = S0 > 0. ? (float)(2. / S0) : 0.f;
    }
    r.loss = r.part1 + r.part2;
    return r;
}

}  // namespace wv
