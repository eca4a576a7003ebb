// What wv_rank_ap (rank_ap.hip) and its host twin (host_rank_ap.cpp) share: the limits, the argument rules -- every refusal
// is answered here, before any pointer is read and before any HIP call --, the workspace layout, the per-pair term R_ij
// with its derivative, and the record a positive leaves behind.  No HIP header is included: a plain C++ compiler can take
// this file.
//
// SmoothAP / SupAP (main/losses/smooth_rank_ap.py) for one query row q, written out in include/wvhash.h: every positive i
// of the row ranks itself against all columns j through R(S[q,j] - S[q,i]); rk_i = 1 + sum R, prk_i = 1 + sum R w,
// AP_q = mean of f_i = prk_i / rk_i.  The gradient of AP_q w.r.t. S[q,j] collects g_ij = (w_ij - f_i) / (rk_i n) R'_ij over
// the positives, that w.r.t. S[q,i] minus the sum of g_ij over j -- which is (sum R' w - f_i sum R') / (rk_i n), so the pass
// that forms rk_i and prk_i sums R' and R' w beside them and the positive's own entry needs no pass of its own.
#pragma once
#include <math.h>
#include <stdint.h>

#include "twin.hpp"

namespace wv {

constexpr int kRankApMax = WV_RANK_AP_COLS_MAX;                 // rows and columns
constexpr int kRankApMaxWords = (kRankApMax + 63) / 64;         // 64-bit words of a bit row

inline int rank_ap_words(int M) { return (M + 63) / 64; }
// workspace: the bit rows of T [B][words], then (quick form) those of LM = (T T^t > 0)
inline size_t rank_ap_bits_bytes(int B, int M) { return (size_t)B * rank_ap_words(M) * sizeof(uint64_t); }
inline size_t rank_ap_ws_bytes(int B, int M, int form)
{
    if (B < 1 || M < 1) return 0;
    return rank_ap_bits_bytes(B, M) * (form == WV_RANK_AP_QUICK ? 2 : 1);
}

// wv_rank_ap[_cpu].  what: the entry point's name in the message; device: the workspace is part of the call
inline int rank_ap_args(const char *what, const void *scores, const void *target, int B, int M, const wv_rank_ap_params *p,
                        const void *ap, bool device, const void *ws, size_t ws_bytes)
{
    if (!scores) WV_FAIL(WV_EINVAL, "%s: scores is null", what);
    if (!target) WV_FAIL(WV_EINVAL, "%s: target is null", what);
    if (!p) WV_FAIL(WV_EINVAL, "%s: params is null", what);
    if (!ap) WV_FAIL(WV_EINVAL, "%s: ap is null", what);
    if (B < 1) WV_FAIL(WV_EINVAL, "%s: B=%d must be >= 1", what, B);
    if (M < 1) WV_FAIL(WV_EINVAL, "%s: M=%d must be >= 1", what, M);
    if (!(p->kind == WV_RANK_AP_SMOOTH || p->kind == WV_RANK_AP_SUP))
        WV_FAIL(WV_EINVAL, "%s: kind=%d (supported: WV_RANK_AP_SMOOTH, WV_RANK_AP_SUP)", what, p->kind);
    if (!(p->form == WV_RANK_AP_QUICK || p->form == WV_RANK_AP_GENERAL))
        WV_FAIL(WV_EINVAL, "%s: form=%d (supported: WV_RANK_AP_QUICK, WV_RANK_AP_GENERAL)", what, p->form);
    if (p->form == WV_RANK_AP_QUICK && B != M)
        WV_FAIL(WV_EINVAL, "%s: the quick form needs a square input, got B=%d M=%d", what, B, M);
    if (!(p->tau > 0.f)) WV_FAIL(WV_EINVAL, "%s: tau=%g must be > 0", what, (double)p->tau);
    if (M > kRankApMax) WV_FAIL(WV_ENOTSUP, "%s: M=%d above WV_RANK_AP_COLS_MAX=%d columns", what, M, kRankApMax);
    if (B > kRankApMax) WV_FAIL(WV_ENOTSUP, "%s: B=%d above WV_RANK_AP_COLS_MAX=%d rows", what, B, kRankApMax);
    if (device) {
        if (!ws) WV_FAIL(WV_EINVAL, "%s: workspace is null", what);
        if (ws_bytes < rank_ap_ws_bytes(B, M, p->form))
            WV_FAIL(WV_EINVAL, "%s: workspace of %zu bytes, %zu needed (wv_rank_ap_workspace_bytes)", what, ws_bytes,
                    rank_ap_ws_bytes(B, M, p->form));
        if (reinterpret_cast<uintptr_t>(ws) & 15) WV_FAIL(WV_EINVAL, "%s: workspace must be 16-byte aligned", what);
    }
    return WV_OK;
}

struct RankTerm {
    float R, dR;      // R(d) and its derivative
};

// sigma_tau(d) = 1 / (1 + exp(clamp(-d / tau, -50, 50))).  With e = exp(x): sigma = 1 / (1 + e) and 1 - sigma = e sigma, no
// difference of nearly equal numbers; the clamp keeps e within fp32 (e^50 = 5.2e21).  Outside the clamp the derivative is 0.
WV_HD RankTerm rank_sigmoid(float d, float tau)
{
    const float x = -d / tau;
    const bool inside = x >= -50.f && x <= 50.f;
    const float e = expf(fminf(fmaxf(x, -50.f), 50.f));
    const float s = 1.f / (1.f + e);
    RankTerm t;
    t.R = s;
    t.dR = inside ? s * (e * s) / tau : 0.f;
    return t;
}

// One pair.  d = S[q,j] - S[q,i]; tgt: the pair's target bit (used by SupAP only)
WV_HD RankTerm rank_term(const wv_rank_ap_params &p, float d, bool tgt)
{
    if (p.kind == WV_RANK_AP_SMOOTH) return rank_sigmoid(d, p.tau);
    RankTerm t;
    if (tgt) {
        t.R = d >= 0.f ? 1.f : 0.f, t.dR = 0.f;              // Heaviside, H(0) = 1
        return t;
    }
    if (d > p.delta && d > 0.f) {
        t.R = p.rho * (d - p.delta) + p.offset, t.dR = p.rho;
        return t;
    }
    t = rank_sigmoid(d, p.tau);
    if (d > 0.f) t.R += p.start;
    return t;
}

// What a positive i of row q leaves for the gradient pass and the row's AP
struct RankApRecord {
    float f;          // prk_i / rk_i
    float c;          // 1 / (rk_i n)
    float own;        // sum_{j != i} g_ij: subtracted from the gradient entry of column i
};

// sR, sRw, sD, sDw: the sums over j != i of R, R w, R', R' w;  n = |P|
WV_HD RankApRecord rank_ap_record(float sR, float sRw, float sD, float sDw, int n)
{
    const float rk = 1.f + sR, prk = 1.f + sRw;
    RankApRecord r;
    r.f = prk / rk;
    r.c = 1.f / (rk * (float)n);
    r.own = (sDw - r.f * sD) * r.c;
    return r;
}

// g_ij for j != i
WV_HD float rank_ap_coeff(const RankApRecord &r, bool w, float dR) { return ((w ? 1.f : 0.f) - r.f) * r.c * dR; }

}  // namespace wv
