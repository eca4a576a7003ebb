// Legacy lifting-scheme DWT (CustomTransform: HaarLifting / Cdf97Lifting) and the ToTensor / Normalize conversion in front of
// it: the arithmetic shared by the gfx950 kernels (lifting.hip, lifting_batched.hip) and the host twin (host_lifting.cpp).
//
// One level = a 1-D lifting pass along H (even / odd ROWS), then along W, both with zero-padded shifts ('constant' pad of the
// shifted operand at every lifting step, not a signal extension): an intermediate (od1, ev1, od2) whose pair index lies
// outside the signal's [0, n) is ZERO.  LL = s.s, LH = d rows of s columns, HL = s rows of d columns, HH = d.d, then the 2-D
// scales (1/sqrt(2)^2, 1, 1, sqrt(2)).  Every product and sum is rounded separately and in the reference's order, so the
// result is bit-identical to the reference's float32 torch ops: every user is compiled with -ffp-contract=off
// (csrc/Makefile), and the functions switch contraction off for themselves where the compiler honours the pragma.
//
// Conversion of one sample (wv_lift_images): t = (float)x / 255.0f (ToTensor's .div(255): a true division), then
// v = (t - mean[c]) / std[c] (Normalize's sub_ / div_: a subtraction and a true division), each rounded to fp32.  A byte has
// 256 values: both users turn the chain into a 256 x C table once (the twin per call, the kernel per workgroup in LDS).
#pragma once
#include <stdint.h>

#include "twin.hpp"

namespace wv {
namespace lift {

constexpr int kHaar = 0, kCdf97 = 1;
constexpr int kMaxChannels = 4;     // C of wv_lift_images: the kernel stages a tile's bytes of all channels and their tables in LDS
constexpr int kMaxLevels = 16;
// wv_lift_images' tile: kTilePairsH x kTilePairsW output samples of every band = 2x that in input samples (+ halo for cdf 9/7)
constexpr int kTilePairsH = 8, kTilePairsW = 64;
constexpr int kHaloPairs = 2;       // cdf 9/7: pair i reads pairs i - 2 .. i + 2 (samples 2i - 4 .. 2i + 4)

struct Consts {
    float a1, a2, a3, a4, k, rk;    // cdf 9/7 steps and scale; for haar k = sqrt(2), rk = 1/sqrt(2)
    float sc_ll, sc_hh;             // 2-D scales of LL and HH (LH, HL: 1)
};

// the constants as the reference rounds them: doubles converted to fp32 once (host code: the kernels take the struct by value)
inline Consts consts(int basis)
{
    const double r2 = 1.4142135623730951;                       // sqrt(2.0) in double
    Consts c;
    if (basis == kHaar) {
        c = {0.f, 0.f, 0.f, 0.f, (float)r2, (float)(1.0 / r2), 0.f, 0.f};
    } else {
        const double k = 1.149604398;
        c = {(float)-1.58613432, (float)-0.05298011854, (float)0.8829110762, (float)0.4435068522, (float)k, (float)(1.0 / k), 0.f, 0.f};
    }
    c.sc_ll = (float)(1.0 / (r2 * r2));
    c.sc_hh = (float)r2;
    return c;
}

// length of one axis as a level sees it (HaarLifting pads to even, Cdf97Lifting to a multiple of 4, with zeros at the end)
WV_HD int padded(int n, int basis) { return basis == kHaar ? n + (n & 1) : (n + 3) & ~3; }

// length of one axis after `levels` levels
WV_HD int out_size(int n, int basis, int levels)
{
    for (int l = 0; l < levels; ++l) n = padded(n, basis) / 2;
    return n;
}

// s and d of the N consecutive pairs i .. i + N - 1 of a 1-D signal of n pairs.  ev(j) / od(j) = samples 2j / 2j + 1; they
// are only called with 0 <= j < n, an index outside [0, n) stands for the zero pad of the lifting step.  Neighbouring pairs
// share their intermediates: every intermediate is formed once, by the same operations in the same order whatever N is, so
// the results do not depend on N.  (Pairs at or beyond n come out as whatever the zero rule yields; callers drop them.)
template <int BASIS, int N, class Ev, class Od>
WV_HD void pairs(Ev ev, Od od, int n, int i, const Consts &c, float (&s)[N], float (&d)[N])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if constexpr (BASIS == kHaar) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int j = i + u;
            const bool in = j < n;
            const float e = in ? ev(j) : 0.f;
            const float od1 = (in ? od(j) : 0.f) + -1.0f * e;
            const float ev1 = e + 0.5f * od1;
            s[u] = c.k * ev1;
            d[u] = c.rk * od1;
        }
    } else {
        // od1 on [i-2, i+N], ev1 on [i-1, i+N], od2 on [i-1, i+N-1], ev2 on [i, i+N-1]
        float e[N + 4];                   // ev(i-2 .. i+N+1)
#pragma unroll
        for (int u = 0; u < N + 4; ++u) { const int j = i - 2 + u; e[u] = (j >= 0 && j < n) ? ev(j) : 0.f; }
        float od1[N + 3];                 // od1(i-2 .. i+N)
#pragma unroll
        for (int u = 0; u < N + 3; ++u) {
            const int j = i - 2 + u;
            od1[u] = (j >= 0 && j < n) ? od(j) + (c.a1 * e[u] + c.a1 * e[u + 1]) : 0.f;
        }
        float ev1[N + 2];                 // ev1(i-1 .. i+N)
#pragma unroll
        for (int u = 0; u < N + 2; ++u) {
            const int j = i - 1 + u;
            ev1[u] = (j >= 0 && j < n) ? e[u + 1] + (c.a2 * od1[u] + c.a2 * od1[u + 1]) : 0.f;
        }
        float od2[N + 1];                 // od2(i-1 .. i+N-1)
#pragma unroll
        for (int u = 0; u < N + 1; ++u) {
            const int j = i - 1 + u;
            od2[u] = (j >= 0 && j < n) ? od1[u + 1] + (c.a3 * ev1[u] + c.a3 * ev1[u + 1]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float ev2 = ev1[u + 1] + (c.a4 * od2[u] + c.a4 * od2[u + 1]);
            s[u] = c.k * ev2;
            d[u] = c.rk * od2[u + 1];
        }
    }
}

// one pair
template <int BASIS, class Ev, class Od>
WV_HD void pair(Ev ev, Od od, int n, int i, const Consts &c, float &s, float &d)
{
    float s1[1], d1[1];
    pairs<BASIS, 1>(ev, od, n, i, c, s1, d1);
    s = s1[0];
    d = d1[0];
}

// how a byte becomes a sample: to_tensor = divide by 255, norm = subtract mean[c], divide by std[c]
struct Convert {
    int to_tensor, norm;
    float mean[kMaxChannels], std[kMaxChannels];
};

// Both divisions must be IEEE-correct on the device as on the host: lifting_batched.o is built with
// -fhip-fp32-correctly-rounded-divide-sqrt spelled out (csrc/Makefile); a reciprocal-multiply division would differ in the
// last bit for constants no test uses.
WV_HD float convert_byte(const Convert &cv, int c, int x)
{
    float t = (float)x;
    if (cv.to_tensor) t = t / 255.0f;
    if (cv.norm) t = (t - cv.mean[c]) / cv.std[c];
    return t;
}

// The part of the argument check that wv_lift_images_check's signature does not carry (to_tensor, mean, std), and the
// Convert it yields; defined beside the check (host_lifting.cpp), called by both entry points.
int convert_args(const char *who, int in_dtype, int C, int to_tensor, const float *mean, const float *std, Convert *cv);

}  // namespace lift
}  // namespace wv
