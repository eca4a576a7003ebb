// One band of the level-n SWT, written as a plain [B][C][H][W] batch (wv_swt2d_band_forward): the sliding kernel of
// swt_slide.hip specialised for a single output stream.
//
// Same scheme -- a persistent workgroup per (image, channel) plane, producer waves that row-filter TH input rows per
// chunk into an LDS ring, consumer waves (thread = column) that stream the column cascade with its tails in registers --
// with everything the other three bands need left out:
//   producers : lower levels are the approximation chain as before; at the last level only the ONE row filter the band
//               needs (lo for cA / cH, hi for cV / cD) is applied and staged
//   ring      : one plane, TH rows x pitch P floats per buffer (half the four-band ring)
//   consumers : the cascade runs on scalars instead of (row-lo, row-hi) pairs, the last level applies the ONE column filter
//               (lo for cA / cV, hi for cH / cD) and there is one store stream
// The band is chosen on the host: the kernel takes the approximation filter `lo` and the last level's row and column
// filters as three tap arrays, so one instantiation per (taps, levels, dtypes, layout) serves all four bands.
// Every output keeps the taps and their order of k_swt_slide (multiply for tap 0, then fma, m = 1..L-1): scalar and
// packed fp32 fma are the same IEEE operation, so each element equals the four-band kernel's bit for bit.
#include "swt_slide.hpp"

namespace wv {

// Waves per SIMD the kernel is compiled for; workgroups per CU = kBandMinW / 2 (a workgroup is 8 waves on 4 SIMDs).
#ifndef WV_BAND_MINW
#define WV_BAND_MINW 4
#endif
constexpr int kBandMinW = WV_BAND_MINW;

struct BandGeom {
    int B, C, H, W;
    int P, nrun, coal, nxcd;   // as in SlideGeom; the output is one [B][C][H][W] batch: plane (b, c) starts at (b*C + c) * H*W
};

template <int L>
struct BandTaps {
    float lo[L];    // levels below the last, both directions
    float row[L];   // last level along x
    float col[L];   // last level along y
};

template <int L, int NLEV, int R, int TH, int NH, int MINW, typename InT, int LAYOUT, bool BF16>
__global__ __launch_bounds__(2 * NH, MINW) void k_swt_band(const InT *__restrict__ in, void *__restrict__ out, BandGeom g,
                                                           BandTaps<L> taps)
{
    using OutT = typename std::conditional<BF16, __hip_bfloat16, float>::type;
    const int P = g.P, W = g.W, H = g.H;
    const uint32_t band = (uint32_t)H * W;
    const ChunkRing<TH, 1> ring(P, H + VStep<L, NLEV, TH>::HALO);
    const PlaneSchedule sched(g);
    const bool is_h = threadIdx.x >= NH;                  // wave-uniform role
    const int t = is_h ? threadIdx.x - NH : threadIdx.x;
    // LDS row layout: run j writes its R outputs as R / 4 float4s, float4 q4 of every run side by side, so consecutive
    // lanes (= consecutive runs) write consecutive 16-byte slots: column x = j*R + 4*q4 + e lives at float
    // q4*(4*nrun) + 4*j + e of its row
    const int qstride = 4 * g.nrun;
    if (is_h) {
#define WV_STAGE_ROW(PROW, CASC, w) do {                  /* a finished row -> LDS */ \
            float *prow = PROW; \
            _Pragma("unroll") \
            for (int q4 = 0; q4 < R / 4; ++q4) { \
                float4 v4; \
                v4.x = CASC::last(w, taps.row, 4 * q4 + 0); v4.y = CASC::last(w, taps.row, 4 * q4 + 1); \
                v4.z = CASC::last(w, taps.row, 4 * q4 + 2); v4.w = CASC::last(w, taps.row, 4 * q4 + 3); \
                *reinterpret_cast<float4 *>(prow + q4 * qstride) = v4; \
            } \
        } while (0)
        WV_SLIDE_PRODUCER(taps.lo, WV_STAGE_ROW);
#undef WV_STAGE_ROW
    } else {
        // ------------------------------------------------------------------ consumer: pass V (see k_swt_slide)
        const bool active = t < W;
        __builtin_amdgcn_s_setprio(kConsumerPrio);   // the critical role issues first
        const int tp = ((t % R) / 4) * qstride + (t / R) * 4 + (t & 3);   // this column's slot in the permuted LDS row
        using VS = VStep<L, NLEV, TH, float>;
        for (int q = sched.first; q < sched.nq; q += sched.step) {
            OutT *oplane = reinterpret_cast<OutT *>(out) + (size_t)sched.at(q).plane * band;
            float tail[VS::HALO];
#pragma unroll
            for (int i = 0; i < VS::HALO; ++i) tail[i] = 0.f;
            __syncthreads();       // chunk 0 produced
            for (int k = 0; k < ring.nchunks; ++k) {
                const int y0 = k * TH - VS::HALO;          // first output row this chunk emits (uniform)
                if (active) {
                    const float *col = ring.buffer(k) + tp;
                    float cur[TH];
#pragma unroll
                    for (int i = 0; i < TH; ++i) cur[i] = col[i * ring.pitch()];
                    VS::template lower<1>(cur, tail, taps.lo);
                    if (y0 + TH <= 0) {                    // nothing to emit yet: only advance the state
                        VS::prime_last(cur, tail);
                    } else {
                        const uint32_t o0 = (uint32_t)t * (uint32_t)sizeof(OutT);   // < 2^32 (slide_fits)
                        VS::last1(cur, tail, taps.col, [&](int i, float a) {
                            const int y = y0 + i;
                            if (y >= 0 && y < H) store_row(oplane + (size_t)y * W, o0, (OutT)a);   // uniform row pointer
                        });
                    }
                }
                __syncthreads();   // buffer k & 1 drained, buffer (k+1) & 1 full
            }
        }
    }
}

template <int L, int NLEV>
static int launch_band(const SwtShape &s, const void *in, void *out, const BandGeom &g, size_t lds, int band,
                       const float *lo, const float *hi, hipStream_t st)
{
    // cA = (row lo, col lo), cH = (row lo, col hi), cV = (row hi, col lo), cD = (row hi, col hi)
    const float *row = band >= 2 ? hi : lo, *col = (band & 1) ? hi : lo;
    BandTaps<L> taps;
    for (int i = 0; i < L; ++i) { taps.lo[i] = lo[i]; taps.row[i] = row[i]; taps.col[i] = col[i]; }
    return slide_io_dispatch(s, [&](auto in_t, auto layout, auto bf16) {
        using InT = decltype(in_t);
        return slide_launch<InT, layout()>(k_swt_band<L, NLEV, kSlideR, kSlideTH, kSlideNT, kBandMinW, InT, layout(), bf16()>,
                                           "k_swt_band", "swt band", kBandMinW, in, out, g, lds, taps, st);
    });
}

// `s` passed slide_fits(); band is 0..3
int swt_band_launch(const SwtShape &s, const void *in, void *out, int band, const float *lo, const float *hi,
                    hipStream_t st)
{
    const SlideRing r = slide_ring(s.W, 1);
    BandGeom g{};
    g.B = s.B; g.C = s.C; g.H = s.H; g.W = s.W;
    g.nrun = r.nrun; g.P = r.P;
#define WV_CFG(LL, NN) if (s.L == LL && s.level == NN) return launch_band<LL, NN>(s, in, out, g, r.lds, band, lo, hi, st);
    WV_SWT_CONFIGS(WV_CFG)
#undef WV_CFG
    WV_FAIL(WV_ENOTSUP, "swt band: %d taps at level %d", s.L, s.level);   // unreachable after slide_fits()
}

}  // namespace wv
