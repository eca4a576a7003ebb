// 2-D SWT: the device helpers its kernels share and the host interface of each implementation.
//   swt_slide.hip : sliding-window persistent kernel, full-width rows (the hot path)
//   swt_band.hip  : the same scheme for ONE band written as a plain image batch (single-band models)
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

// The same cascade for a line cut into runs of R outputs, one run per lane, when every lane of the wave runs it together.
// The stencil is one-sided -- level l output i reads inputs i .. i + (L-1)*2^(l-1) -- so a run OWNS outputs 0 .. R-1 of
// every level below the last and takes the (L-1)*2^l values the next level reads past them from the run to its right
// (ds_bpermute through `right`, a lane byte address): every level value is computed once per line instead of once per
// run that reads it.  w[] holds R + L-1 inputs on entry; lower() leaves the R + (L-1)*2^(NLEV-1) inputs of the last
// level.  Each output keeps the taps and their order of Cascade, so it keeps its bits.
template <int L, int NLEV, int R>
struct RunCascade {
    static constexpr int NPIX = R + (L - 1);
    static constexpr int NW = R + (L - 1) * (1 << (NLEV - 1));
    static_assert((L - 1) * (1 << (NLEV - 1)) < R, "a level's halo must come from one neighbouring run");

    template <int LEV>
    static __device__ __forceinline__ void lower(float (&w)[NW], const float (&lo)[L], int right)
    {
        if constexpr (LEV < NLEV) {
            constexpr int S = 1 << (LEV - 1);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                float a = lo[0] * w[i + S * (L - 1)];
#pragma unroll
                for (int m = 1; m < L; ++m) a = fmaf(lo[m], w[i + S * (L - 1 - m)], a);
                w[i] = a;
            }
#pragma unroll
            for (int i = 0; i < 2 * S * (L - 1); ++i)
                w[R + i] = __int_as_float(__builtin_amdgcn_ds_bpermute(right, __float_as_int(w[i])));
            lower<LEV + 1>(w, lo, right);
        }
    }
    static __device__ __forceinline__ float last(const float (&w)[NW], const float (&f)[L], int i)
    {
        constexpr int S = 1 << (NLEV - 1);
        float a = f[0] * w[i + S * (L - 1)];
#pragma unroll
        for (int m = 1; m < L; ++m) a = fmaf(f[m], w[i + S * (L - 1 - m)], a);
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

// ------------------------------------------------------------------------------- sliding kernels
// What k_swt_slide (swt_slide.hip, four bands) and k_swt_band (swt_band.hip, one band) share.
// The one configuration every (taps, levels) instantiation uses: runs of R columns, TH rows per step, NT threads per
// role (W <= NT), MINW workgroups per CU.
constexpr int kSlideR = 16, kSlideTH = 16, kSlideNT = 256, kSlideMinW = 4;
constexpr int kPitchPad = 4;      // LDS ring pitch = nrun * R + 4 floats
// A/B on MI355X in one session, db2 level 3, 2048 images: consumer (column) waves at raised issue priority: 1.148 ms vs
// 1.19 ms at equal priority (they are the critical role)
constexpr int kConsumerPrio = 2;
constexpr int kXcds = 8;          // workgroup w runs on XCD w % 8 (hardware round-robin)

// Streaming form of the cascade for pass V: a thread keeps, per column, the last (L-1)*2^(l-1)
// inputs of every level l in registers ("tails", HALO values in all), so each step costs exactly
// L MACs per level per new row -- no halo recompute -- and emits outputs delayed by HALO rows.
// The arithmetic per output is identical to Cascade (same taps, same order).
// It runs on (row-lo, row-hi) PAIRS: the two row-filtered planes go through identical arithmetic, so the
// consumer keeps them as 2-vectors and every multiply-add becomes one v_pk_fma_f32 -- half the instructions a
// wave has to issue for the same (bitwise identical) result.  The LDS ring holds the planes interleaved.
using f32x2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2 fma_s(float s, f32x2 x, f32x2 a)
{
    const f32x2 sv = {s, s};
    return __builtin_elementwise_fma(sv, x, a);
}
__device__ __forceinline__ float fma_s(float s, float x, float a) { return fmaf(s, x, a); }

// The single-band kernel (swt_band.hip) runs the same cascade on one plane: V = float, last1() for its one column filter.
template <int L, int NLEV, int N, typename V = f32x2>
struct VStep {
    using T = V;
    static constexpr int HALO = (L - 1) * ((1 << NLEV) - 1);
    // levels LEV .. NLEV-1: cur[] holds N new level-LEV inputs on entry, N new level-NLEV inputs on exit
    template <int LEV>
    static __device__ __forceinline__ void lower(T (&cur)[N], T (&tail)[HALO], const float (&lo)[L])
    {
        if constexpr (LEV < NLEV) {
            constexpr int S = 1 << (LEV - 1), TT = (L - 1) * S, OFF = (L - 1) * (S - 1);
            T seq[TT + N];
#pragma unroll
            for (int i = 0; i < TT; ++i) seq[i] = tail[OFF + i];
#pragma unroll
            for (int i = 0; i < N; ++i) seq[TT + i] = cur[i];
#pragma unroll
            for (int t = 0; t < N; ++t) {
                T a = lo[0] * seq[t + S * (L - 1)];
#pragma unroll
                for (int m = 1; m < L; ++m) a = fma_s(lo[m], seq[t + S * (L - 1 - m)], a);
                cur[t] = a;
            }
#pragma unroll
            for (int i = 0; i < TT; ++i) tail[OFF + i] = seq[N + i];
            lower<LEV + 1>(cur, tail, lo);
        }
    }
    // last level: seq = tail ++ cur; out(t) for t < N; tail updated
    template <typename Emit>
    static __device__ __forceinline__ void last(const T (&cur)[N], T (&tail)[HALO], const float (&lo)[L],
                                                const float (&hi)[L], Emit emit)
    {
        constexpr int S = 1 << (NLEV - 1), TT = (L - 1) * S, OFF = (L - 1) * (S - 1);
        T seq[TT + N];
#pragma unroll
        for (int i = 0; i < TT; ++i) seq[i] = tail[OFF + i];
#pragma unroll
        for (int i = 0; i < N; ++i) seq[TT + i] = cur[i];
#pragma unroll
        for (int t = 0; t < N; ++t) {
            T a = lo[0] * seq[t + S * (L - 1)], d = hi[0] * seq[t + S * (L - 1)];
#pragma unroll
            for (int m = 1; m < L; ++m) {
                a = fma_s(lo[m], seq[t + S * (L - 1 - m)], a);
                d = fma_s(hi[m], seq[t + S * (L - 1 - m)], d);
            }
            emit(t, a, d);
        }
#pragma unroll
        for (int i = 0; i < TT; ++i) tail[OFF + i] = seq[N + i];
    }
    // last level of one band: the one column filter f, same taps in the same order
    template <typename Emit>
    static __device__ __forceinline__ void last1(const T (&cur)[N], T (&tail)[HALO], const float (&f)[L], Emit emit)
    {
        constexpr int S = 1 << (NLEV - 1), TT = (L - 1) * S, OFF = (L - 1) * (S - 1);
        T seq[TT + N];
#pragma unroll
        for (int i = 0; i < TT; ++i) seq[i] = tail[OFF + i];
#pragma unroll
        for (int i = 0; i < N; ++i) seq[TT + i] = cur[i];
#pragma unroll
        for (int t = 0; t < N; ++t) {
            T a = f[0] * seq[t + S * (L - 1)];
#pragma unroll
            for (int m = 1; m < L; ++m) a = fma_s(f[m], seq[t + S * (L - 1 - m)], a);
            emit(t, a);
        }
#pragma unroll
        for (int i = 0; i < TT; ++i) tail[OFF + i] = seq[N + i];
    }
    // warm-up: only refresh the last level's tail
    static __device__ __forceinline__ void prime_last(const T (&cur)[N], T (&tail)[HALO])
    {
        constexpr int S = 1 << (NLEV - 1), TT = (L - 1) * S, OFF = (L - 1) * (S - 1);
        T seq[TT + N];
#pragma unroll
        for (int i = 0; i < TT; ++i) seq[i] = tail[OFF + i];
#pragma unroll
        for (int i = 0; i < N; ++i) seq[TT + i] = cur[i];
#pragma unroll
        for (int i = 0; i < TT; ++i) tail[OFF + i] = seq[N + i];
    }
};

// LAYOUT: 0 = NCHW, 1 = NHWC with C == 3.  One aligned 4-pixel group of channel c, raw.
template <typename InT, int LAYOUT>
struct SRaw {
    uint32_t d[sizeof(InT) == 1 ? (LAYOUT == 1 ? 3 : 1) : 4];
};

// `img` = uniform base of the (b) image [NHWC] or of the (b, c) plane [NCHW]; off = lane offset in elements
template <typename InT, int LAYOUT>
__device__ __forceinline__ SRaw<InT, LAYOUT> s_fetch4(const InT *__restrict__ img, uint32_t pix, int c)
{
    SRaw<InT, LAYOUT> r;
    if constexpr (sizeof(InT) == 1) {
        if constexpr (LAYOUT == 0) {
            r.d[0] = *reinterpret_cast<const uint32_t *>(img + pix);
        } else {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(img + pix * 3u);
            r.d[0] = p[0]; r.d[1] = p[1]; r.d[2] = p[2];
        }
    } else {
        float4 v;
        if constexpr (LAYOUT == 0) {
            v = *reinterpret_cast<const float4 *>(img + pix);
        } else {
            const InT *p = img + pix * 3u + c;
            v = make_float4(p[0], p[3], p[6], p[9]);
        }
        r.d[0] = __float_as_uint(v.x); r.d[1] = __float_as_uint(v.y);
        r.d[2] = __float_as_uint(v.z); r.d[3] = __float_as_uint(v.w);
    }
    return r;
}

template <typename InT, int LAYOUT>
__device__ __forceinline__ float4 s_convert4(const SRaw<InT, LAYOUT> &r, int c)
{
    if constexpr (sizeof(InT) == 1) {
        if constexpr (LAYOUT == 1) return rgb4_to_unit(r.d[0], r.d[1], r.d[2], c);
        else return u8x4_to_unit(r.d[0]);
    } else {
        return make_float4(__uint_as_float(r.d[0]), __uint_as_float(r.d[1]), __uint_as_float(r.d[2]),
                           __uint_as_float(r.d[3]));
    }
}

// Store through "SGPR base + 32-bit lane offset" addressing (global_store ... saddr): the row pointer is
// wave-uniform, so no per-store 64-bit vector address arithmetic is needed.  hipcc builds the address in
// VGPRs for this pattern, hence the explicit instruction.  Only V waves store and they issue no vector
// loads in their loop, so the compiler's vmcnt bookkeeping is unaffected.
__device__ __forceinline__ void store_row(float *row_uniform, uint32_t byte_off, float v)
{
#ifdef WV_SWT_NOSTORE   // diagnostic build: arithmetic only (the store survives only for a value that never occurs)
    if (__float_as_uint(v) == byte_off * 0x9E3779B1u + 0x7fc12345u)
        *reinterpret_cast<float *>(reinterpret_cast<char *>(row_uniform) + byte_off) = v;
    return;
#endif
    asm volatile("global_store_dword %0, %1, %2" : : "v"(byte_off), "v"(v), "s"(row_uniform) : "memory");
}
__device__ __forceinline__ void store_row(__hip_bfloat16 *row_uniform, uint32_t byte_off, __hip_bfloat16 v)
{
    *reinterpret_cast<__hip_bfloat16 *>(reinterpret_cast<char *>(row_uniform) + byte_off) = v;
}


// ------------------------------------------------------------------------------- host side
// One call of wv_swt2d_forward[_ex]: L taps, `level` levels, WV_DT_* dtypes, WV_LAYOUT_* input layout.
struct SwtShape {
    int B, C, H, W, level, L;
    int in_dtype, out_dtype, in_layout;
};

// LDS ring of width W holding `planes` row-filtered planes (2: lo and hi, the four-band kernel; 1: the single-band
// kernel): runs per row, pitch, bytes.  The planner (slide_fits) and the launches use this one computation.
struct SlideRing {
    int nrun, P;
    size_t lds;
};
inline SlideRing slide_ring(int W, int planes = 2)
{
    SlideRing r;
    r.nrun = (int)ceil_div(W, kSlideR);
    r.P = r.nrun * kSlideR + kPitchPad;                         // multiple of 4; rows hold whole runs
    r.lds = (size_t)2 * planes * kSlideTH * r.P * sizeof(float);   // 2 buffers x planes
    return r;
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
