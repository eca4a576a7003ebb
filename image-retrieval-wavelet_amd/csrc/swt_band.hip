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
#include "swt.hpp"
#include <type_traits>

namespace wv {

// Waves per SIMD the kernel is compiled for; workgroups per CU = kBandMinW / 2 (a workgroup is 8 waves on 4 SIMDs).
#ifndef WV_BAND_MINW
#define WV_BAND_MINW 4
#endif
constexpr int kBandMinW = WV_BAND_MINW;

struct BandGeom {
    int B, C, H, W;
    int P;          // ring pitch in floats
    int nrun;       // runs per row = ceil(W / R)
    int coal;       // planar uint8, W % 16 == 0: producers load every pixel once, coalesced (as in k_swt_slide)
    int nxcd;       // 8: workgroups w, w+8, ... (one XCD) share images; 1: plain striding
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
    using CH = Cascade<L, NLEV, R>;
    using Raw = SRaw<InT, LAYOUT>;
    using OutT = typename std::conditional<BF16, __hip_bfloat16, float>::type;
    constexpr int HALO = CH::HALO;
    constexpr int HB = (L / 2 - 1) * ((1 << NLEV) - 1);
    constexpr int HBa = (HB + 3) / 4 * 4;
    constexpr int NG = (HBa - HB + CH::NIN + 3) / 4;      // 4-pixel groups one run loads
    static_assert(R % 4 == 0, "run length must be a multiple of 4");
    extern __shared__ float4 band_ring4[];
    float *ring = reinterpret_cast<float *>(band_ring4);  // [2 buffers][TH][P]
    const int P = g.P, W = g.W, H = g.H;
    const int buf_sz = TH * P;
    const int nchunks = (H + HALO + TH - 1) / TH;         // the cascade consumes H + HALO rows per plane
    const uint32_t band = (uint32_t)H * W;
    // plane schedule of k_swt_slide: image b belongs to XCD b % nxcd, its planes to neighbouring workgroups of that XCD
    const int xcd = blockIdx.x % g.nxcd, wg_in_xcd = blockIdx.x / g.nxcd, wgs_per_xcd = gridDim.x / g.nxcd;
    const int nq = g.B > xcd ? (g.B - xcd + g.nxcd - 1) / g.nxcd * g.C : 0;   // planes this XCD owns
    const bool is_h = threadIdx.x >= NH;                  // wave-uniform role
    const int t = is_h ? threadIdx.x - NH : threadIdx.x;
    // LDS row layout: run j writes its R outputs as R / 4 float4s, float4 q4 of every run side by side, so consecutive
    // lanes (= consecutive runs) write consecutive 16-byte slots: column x = j*R + 4*q4 + e lives at float
    // q4*(4*nrun) + 4*j + e of its row
    const int qstride = 4 * g.nrun;
    if (is_h) {
        // ------------------------------------------------------------------ producer: pass H (see k_swt_slide)
        int rr = t / g.nrun, j = t - rr * g.nrun;
        bool active = t < TH * g.nrun;
        int lane_left = 0, lane_right = 0, rr_ld = 0, wrow0 = 0;
        if (g.coal) {
            const int l = t & 63, rpw = 64 / g.nrun, lr = l / g.nrun;
            j = l - lr * g.nrun;
            wrow0 = (t >> 6) * rpw;                                              // first row of this wave
            rr = wrow0 + lr;
            active = lr < rpw && rr < TH;
            rr_ld = min(rr, TH - 1);                                             // spare lanes load a valid row too
            lane_left = (lr * g.nrun + (j == 0 ? g.nrun - 1 : j - 1)) * 4;       // byte addresses for ds_bpermute
            lane_right = (lr * g.nrun + (j == g.nrun - 1 ? 0 : j + 1)) * 4;      // (periodic: the row wraps onto itself)
            if (lr >= rpw) lane_left = lane_right = 0;
        }
        for (int q = wg_in_xcd; q < nq; q += wgs_per_xcd) {
            const int m = q / g.C, c = q - m * g.C, b = xcd + g.nxcd * m, pc = b * g.C + c;
            const InT *img = LAYOUT == 0 ? in + (size_t)pc * band : in + (size_t)b * band * 3;
            Raw raw[NG];
            auto fetch = [&](int chunk) {
                // input row of virtual row v = chunk*TH + rr is y = v - HB (wrapped; rows past H + HA wrap too)
                int y = chunk * TH + rr - HB;
                y = y >= H ? y - H : y;
                const uint32_t row = (uint32_t)wrap_once(y, H) * (uint32_t)W;
                const int gx0 = j * R - HBa;
#pragma unroll
                for (int k = 0; k < NG; ++k)
                    raw[k] = s_fetch4<InT, LAYOUT>(img, row + (uint32_t)wrap_once(gx0 + 4 * k, W), c);
            };
            constexpr bool CAN_COAL = sizeof(InT) == 1 && LAYOUT == 0 && R == 16 && NG * 4 - HBa <= 32;
            uint32_t own[4] = {0, 0, 0, 0};
            auto issue_row = [&](int chunk) {       // every lane of the wave (the exchange below reads all of them)
                int y = chunk * TH + rr_ld - HB;
                y = y >= H ? y - H : y;
                const uint4 v4 = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(img) +
                                                                  (size_t)wrap_once(y, H) * W + j * R);
                own[0] = v4.x; own[1] = v4.y; own[2] = v4.z; own[3] = v4.w;
            };
            const bool coal = CAN_COAL && g.coal;   // uniform
            if (coal) {
                if constexpr (CAN_COAL) {
                    issue_row(0);
                    for (int k = 0; k < nchunks; ++k) {
                        using RC = RunCascade<L, NLEV, R>;
                        constexpr int NGC = (HBa - HB + RC::NPIX + 3) / 4;     // 4-pixel groups level 1 reads
                        static_assert(HBa <= 16 && 4 * NGC - HBa <= 32, "the pixel window must end in the neighbouring runs");
                        const int wrow = __builtin_amdgcn_readfirstlane(wrow0);             // wave-uniform
                        const bool live = wrow < TH && k * TH + wrow < H + HALO;
                        if (live) {
                            float w[RC::NW];
                            // pixels [16j - HBa, 16j - HBa + 4 NGC): left neighbour | own | right neighbour
                            float v[NGC * 4];
#pragma unroll
                            for (int kk = 0; kk < NGC; ++kk) {
                                const int gpx = 4 * kk - HBa;                  // compile-time after unrolling
                                uint32_t d;
                                if (gpx < 0)
                                    d = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_left, (int)own[(gpx + 16) / 4]);
                                else if (gpx < 16)
                                    d = own[gpx / 4];
                                else
                                    d = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_right, (int)own[(gpx - 16) / 4]);
                                const float4 p4 = u8x4_to_unit(d);
                                v[4 * kk + 0] = p4.x; v[4 * kk + 1] = p4.y; v[4 * kk + 2] = p4.z; v[4 * kk + 3] = p4.w;
                            }
#pragma unroll
                            for (int i = 0; i < RC::NPIX; ++i) w[i] = v[i + HBa - HB];
                            if (k + 1 < nchunks) issue_row(k + 1);             // flies during this chunk's arithmetic
                            RC::template lower<1>(w, taps.lo, lane_right);
                            if (active && k * TH + rr < H + HALO) {
                                float *prow = ring + (k & 1) * buf_sz + rr * P + 4 * j;
#pragma unroll
                                for (int q4 = 0; q4 < R / 4; ++q4) {
                                    float4 v4;
                                    v4.x = RC::last(w, taps.row, 4 * q4 + 0); v4.y = RC::last(w, taps.row, 4 * q4 + 1);
                                    v4.z = RC::last(w, taps.row, 4 * q4 + 2); v4.w = RC::last(w, taps.row, 4 * q4 + 3);
                                    *reinterpret_cast<float4 *>(prow + q4 * qstride) = v4;
                                }
                            }
                        } else {
                            if (k + 1 < nchunks) issue_row(k + 1);
                        }
                        __syncthreads();   // buffer k & 1 is full; buffer (k+1) & 1 was drained before this barrier
                    }
                }
            } else {
                if (active) fetch(0);
                for (int k = 0; k < nchunks; ++k) {
                    if (active) {
                        float v[NG * 4];
#pragma unroll
                        for (int q2 = 0; q2 < NG; ++q2) {
                            const float4 p4 = s_convert4<InT, LAYOUT>(raw[q2], c);
                            v[4 * q2 + 0] = p4.x; v[4 * q2 + 1] = p4.y; v[4 * q2 + 2] = p4.z; v[4 * q2 + 3] = p4.w;
                        }
                        if (k + 1 < nchunks) fetch(k + 1);              // next chunk's pixels fly during the arithmetic
                        // in-place cascade on v[off ..): element i of the run lives at v[i + off]
                        constexpr int off = HBa - HB;
                        float w[CH::NIN];
#pragma unroll
                        for (int i = 0; i < CH::NIN; ++i) w[i] = v[i + off];
                        CH::template lower<1>(w, taps.lo);
                        float *prow = ring + (k & 1) * buf_sz + rr * P + 4 * j;
#pragma unroll
                        for (int q4 = 0; q4 < R / 4; ++q4) {
                            float4 v4;
                            v4.x = CH::last(w, taps.row, 4 * q4 + 0); v4.y = CH::last(w, taps.row, 4 * q4 + 1);
                            v4.z = CH::last(w, taps.row, 4 * q4 + 2); v4.w = CH::last(w, taps.row, 4 * q4 + 3);
                            *reinterpret_cast<float4 *>(prow + q4 * qstride) = v4;
                        }
                    }
                    __syncthreads();
                }
            }
            __syncthreads();       // pairs with the consumer's last barrier of the plane
        }
    } else {
        // ------------------------------------------------------------------ consumer: pass V
        const bool active = t < W;
        __builtin_amdgcn_s_setprio(kConsumerPrio);   // the critical role issues first
        const int tp = ((t % R) / 4) * qstride + (t / R) * 4 + (t & 3);   // this column's slot in the permuted LDS row
        using VS = VStep<L, NLEV, TH, float>;
        for (int q = wg_in_xcd; q < nq; q += wgs_per_xcd) {
            const int m = q / g.C, pc = (xcd + g.nxcd * m) * g.C + (q - m * g.C);
            OutT *oplane = reinterpret_cast<OutT *>(out) + (size_t)pc * band;
            float tail[HALO > 0 ? HALO : 1];
#pragma unroll
            for (int i = 0; i < HALO; ++i) tail[i] = 0.f;
            __syncthreads();       // chunk 0 produced
            for (int k = 0; k < nchunks; ++k) {
                const int y0 = k * TH - HALO;              // first output row this chunk emits (uniform)
                if (active) {
                    const float *col = ring + (k & 1) * buf_sz + tp;
                    float cur[TH];
#pragma unroll
                    for (int i = 0; i < TH; ++i) cur[i] = col[i * P];
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

template <int L, int NLEV, typename InT, int LAYOUT, bool BF16>
static int launch_band(const void *in, void *out, BandGeom g, size_t lds, const BandTaps<L> &taps, hipStream_t st)
{
    constexpr int R = kSlideR, TH = kSlideTH, NT = kSlideNT, MINW = kBandMinW;
    auto kern = k_swt_band<L, NLEV, R, TH, NT, MINW, InT, LAYOUT, BF16>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) WV_FAIL(WV_EHIP, "swt band: hipFuncSetAttribute(%zu): %s", lds, hipGetErrorString(e));
    }
    static int num_cu = 0;
    if (!num_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
            WV_FAIL(WV_EHIP, "swt band: device query failed");
        num_cu = prop.multiProcessorCount;
    }
    // persistent grid, the rule of launch_slide: workgroups per CU by LDS and by the compiled occupancy, a multiple of
    // the XCD count when the launch has fewer workgroups than planes
    const int by_lds = std::max<int>(1, (int)((size_t)kMaxLdsBytes / (lds + 512)));
    const int per_cu = std::min(by_lds, std::max(1, MINW * 256 / (2 * NT)));
    const int64_t planes = (int64_t)g.B * g.C;
    int64_t grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    g.coal = std::is_same<InT, uint8_t>::value && LAYOUT == 0 && R == 16 && g.W % 16 == 0 && g.nrun <= 16 &&
             (int64_t)g.H * g.W % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    g.nxcd = kXcds;
    if (grid < planes) grid -= grid % g.nxcd;
    if (grid <= 0 || grid % g.nxcd) g.nxcd = 1, grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(2 * NT), lds, st, (const InT *)in, out, g, taps);
    WV_CHECK_LAUNCH("k_swt_band");
    return WV_OK;
}

template <int L, int NLEV>
static int band_types(const SwtShape &s, const void *in, void *out, const BandGeom &g, size_t lds, int band,
                      const float *lo, const float *hi, hipStream_t st)
{
    // cA = (row lo, col lo), cH = (row lo, col hi), cV = (row hi, col lo), cD = (row hi, col hi)
    const float *row = band >= 2 ? hi : lo, *col = (band & 1) ? hi : lo;
    BandTaps<L> taps;
    for (int i = 0; i < L; ++i) { taps.lo[i] = lo[i]; taps.row[i] = row[i]; taps.col[i] = col[i]; }
    const bool nhwc3 = s.in_layout == WV_LAYOUT_NHWC;   // C == 3 (slide_fits)
    const bool bf16 = s.out_dtype == WV_DT_BF16;
#define WV_GO(T, LAY, BF) return launch_band<L, NLEV, T, LAY, BF>(in, out, g, lds, taps, st)
    if (s.in_dtype == WV_DT_U8) {
        if (nhwc3) { if (bf16) WV_GO(uint8_t, 1, true); WV_GO(uint8_t, 1, false); }
        if (bf16) WV_GO(uint8_t, 0, true);
        WV_GO(uint8_t, 0, false);
    }
    if (nhwc3) { if (bf16) WV_GO(float, 1, true); WV_GO(float, 1, false); }
    if (bf16) WV_GO(float, 0, true);
    WV_GO(float, 0, false);
#undef WV_GO
}

// `s` passed slide_fits(); band is 0..3
int swt_band_launch(const SwtShape &s, const void *in, void *out, int band, const float *lo, const float *hi,
                    hipStream_t st)
{
    const SlideRing r = slide_ring(s.W, 1);
    BandGeom g{};
    g.B = s.B; g.C = s.C; g.H = s.H; g.W = s.W;
    g.nrun = r.nrun; g.P = r.P;
#define WV_CFG(LL, NN) if (s.L == LL && s.level == NN) return band_types<LL, NN>(s, in, out, g, r.lds, band, lo, hi, st)
    WV_CFG(4, 3); WV_CFG(2, 1);
    WV_CFG(4, 1); WV_CFG(4, 2); WV_CFG(2, 2); WV_CFG(2, 3); WV_CFG(8, 1); WV_CFG(10, 1);
#undef WV_CFG
    WV_FAIL(WV_ENOTSUP, "swt band: %d taps at level %d", s.L, s.level);   // unreachable after slide_fits()
}

}  // namespace wv
