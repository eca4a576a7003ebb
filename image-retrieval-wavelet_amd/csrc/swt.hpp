// 2-D SWT: the device helpers all its kernels share (cascades, wrapping, pixel conversion), the table of instantiated
// (taps, levels) and the host interface of each implementation.
//   swt_slide.hip : sliding-window persistent kernel, full-width rows (the hot path)
//   swt_band.hip  : the same scheme for ONE band written as a plain image batch (single-band models)
//   swt_slide.hpp : the body of that scheme, which only those two include (roles, plane schedule, launch rule)
//   swt_fused.hip : register-fused two-pass kernel over tiles
//   swt.hip       : tiled 2n-pass LDS kernel, generic per-level kernels, the planner and the entry points
#pragma once
#include "common.hpp"

namespace wv {

template <int L>
struct Taps {
    float lo[L];
    float hi[L];
};

// All NLEV levels of the periodized a-trous filter along one line, in registers.  v[] holds NOUT + HALO inputs;
// lower() applies levels 1 .. NLEV-1 (approximation only) in place -- level l only reads indices >= i -- and
// last() returns level-NLEV output i for filter f.  Taps are accumulated in the reference order (m = 0..L-1, fmaf).
template <int L, int NLEV, int NOUT>
struct Cascade {
    static constexpr int HALO = (L - 1) * ((1 << NLEV) - 1);
    static constexpr int NIN = NOUT + HALO;

    template <int LEV>
    static __device__ __forceinline__ void lower(float (&v)[NIN], const float (&lo)[L])
    {
        if constexpr (LEV < NLEV) {
            constexpr int S = 1 << (LEV - 1);
            constexpr int LEN = NIN - (L - 1) * ((1 << LEV) - 1);
#pragma unroll
            for (int i = 0; i < LEN; ++i) {
                float a = lo[0] * v[i + S * (L - 1)];
#pragma unroll
                for (int m = 1; m < L; ++m) a = fmaf(lo[m], v[i + S * (L - 1 - m)], a);
                v[i] = a;
            }
            lower<LEV + 1>(v, lo);
        }
    }
    static __device__ __forceinline__ float last(const float (&v)[NIN], const float (&f)[L], int i)
    {
        constexpr int S = 1 << (NLEV - 1);
        float a = f[0] * v[i + S * (L - 1)];
#pragma unroll
        for (int m = 1; m < L; ++m) a = fmaf(f[m], v[i + S * (L - 1 - m)], a);
        return a;
    }
};

// v mod n for any v
__device__ __forceinline__ int wrap(int v, int n)
{
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return v;
}

// branch-free v mod n, valid for -n <= v < 2n (in the sliding kernel: W >= R + HALO, H >= TH + 2 * HALO)
__device__ __forceinline__ int wrap_once(int v, int n)
{
    v = v < 0 ? v + n : v;
    return v >= n ? v - n : v;
}

// exact fp32 x / 255 for x in 0..255 (verified exhaustively against IEEE division):
// q = x * r ; e = fma(-q, 255, x) ; q' = fma(e, r, q), r = RN(1/255)
__device__ __forceinline__ float u8_to_unit(float x)
{
    const float r = 0.003921568859368563f;  // 0x3b808081
    const float q = x * r;
    const float e = fmaf(-q, 255.0f, x);
    return fmaf(e, r, q);
}

template <int N>
__device__ __forceinline__ float ubyte(uint32_t d)
{
    return (float)((d >> (8 * N)) & 0xffu);  // -> v_cvt_f32_ubyteN
}

// 4 planar uint8 pixels (one dword) -> [0,1]
__device__ __forceinline__ float4 u8x4_to_unit(uint32_t d)
{
    return make_float4(u8_to_unit(ubyte<0>(d)), u8_to_unit(ubyte<1>(d)), u8_to_unit(ubyte<2>(d)),
                       u8_to_unit(ubyte<3>(d)));
}

// 4 interleaved RGB uint8 pixels = 12 bytes = 3 aligned dwords; channel c sits at bytes c, 3+c, 6+c, 9+c -> [0,1]
__device__ __forceinline__ float4 rgb4_to_unit(uint32_t d0, uint32_t d1, uint32_t d2, int c)
{
    const uint32_t s0 = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)c);
    const uint32_t s1 = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)c);
    const uint32_t s2 = __builtin_amdgcn_alignbyte(0u, d2, (uint32_t)c);
    return make_float4(u8_to_unit(ubyte<0>(s0)), u8_to_unit(ubyte<3>(s0)), u8_to_unit(ubyte<2>(s1)),
                       u8_to_unit(ubyte<1>(s2)));
}

// ------------------------------------------------------------------------------- host side
// One call of wv_swt2d_forward[_ex]: L taps, `level` levels, WV_DT_* dtypes, WV_LAYOUT_* input layout.
struct SwtShape {
    int B, C, H, W, level, L;
    int in_dtype, out_dtype, in_layout;
};

// The (taps, levels) the sliding and the register-fused kernels are instantiated for, X(taps, levels) once per pair: the shipped
// configs (db2 L3 = c1, haar L1 = c0), the other levels of 2 and 4 taps, level 1 of the 8 and 10 taps the studies sweep (db4, bior4.4).
#define WV_SWT_CONFIGS(X) X(4, 3) X(2, 1) X(4, 1) X(4, 2) X(2, 2) X(2, 3) X(8, 1) X(10, 1)
inline bool swt_config(int L, int n)
{
#define WV_IS(LL, NN) if (L == LL && n == NN) return true;
    WV_SWT_CONFIGS(WV_IS)
#undef WV_IS
    return false;
}

// The sliding kernel computes the shape.  On false, `why` (if given) receives the rule the shape breaks.
bool slide_fits(const SwtShape &s, char *why = nullptr, size_t why_len = 0);
// out_layout WV_BANDS_OUTER: out is [4][..][C][H][W] with `band_stride` elements between the bands of one plane
int swt_slide_launch(const SwtShape &s, const void *in, void *out, const float *lo, const float *hi, hipStream_t st,
                     int out_layout = WV_BANDS_INNER, int64_t band_stride = 0);

// One band (0..3 = cA, cH, cV, cD) of a shape slide_fits() accepts, as a plain [B][C][H][W] batch (swt_band.hip).
int swt_band_launch(const SwtShape &s, const void *in, void *out, int band, const float *lo, const float *hi,
                    hipStream_t st);

// The register-fused kernel computes the shape (it ignores dtypes and layout).
bool fused_fits(const SwtShape &s);
int swt_fused_launch(const SwtShape &s, const void *in, void *out, const float *lo, const float *hi, hipStream_t st);

}  // namespace wv
