// Sliding-window SWT kernel for gfx950 (full-width rows, persistent over image planes).
//
// Same register-fused two-pass scheme as swt_fused.hip (all levels of one direction in registers;
// the separable a-trous passes of the two axes commute), restructured for the way the output lies
// in memory: out[b][c][band] is one contiguous H x W block, so a workgroup that owns a whole
// (image, channel) plane and walks down it TH rows at a time writes four pure streams.
//   ring   : LDS ring of RH = TH + HALO rows x 2 planes (row-filtered lo / hi), pitch W + 4
//   step s : pass H on the TH new input rows (each input row is row-filtered exactly once: no
//            vertical halo recompute), barrier, pass V on the RH rows now in the ring -> TH output
//            rows x 4 bands, barrier.  The raw pixels of the next step are fetched into registers
//            before pass V, so global-load latency hides behind the column arithmetic.
//   pass H : thread = (row, run of R columns), pixels wrapped mod W / mod H at load time
//   pass V : thread = (plane, column); lanes = adjacent columns -> each store instruction writes one
//            contiguous row segment, consecutive rows follow each other in memory
// uint8 input is converted exactly (x/255 via fma refinement, verified for all 256 values).
// Schedule, producer role and launch rule: swt_slide.hpp, shared with k_swt_band.  Here: this kernel's stage and consumer.
#include "swt_slide.hpp"

namespace wv {

struct SlideGeom {
    int B, C, H, W;
    int P;          // ring pitch in floats
    int nrun;       // runs per row = ceil(W / R)
    int unused0, unused1, coal, nxcd;   // unused0-2, once in_layout, out_bf16 and stamps, keep the layout (see swt_slide.hpp)
    // output addressing in elements: plane (b, c) starts at (b*C + c) * pstride, its band k at + k * bstride.
    //   [B][C][4][H][W] (reference layout):  pstride = 4*H*W, bstride = H*W
    //   [4][B][C][H][W] (band-major, each band one contiguous NCHW batch):  pstride = H*W, bstride = B*C*H*W
    size_t pstride, bstride;
    void *unused2;
};

// Producer / consumer split inside one workgroup of 2 * NH threads:
//   waves [NH/64, 2*NH/64)  "H waves": fetch the TH input rows of chunk k+1, filter them along x in
//                           registers (all levels) and write lo / hi into LDS buffer (k+1) & 1
//   waves [0, NH/64)        "V waves": thread = column; stream chunk k of both planes from LDS buffer
//                           k & 1 through the per-column cascade (tails in registers) and store the TH
//                           output rows the cascade emits (it lags the input by HALO rows)
// One barrier per chunk hands the buffers over.  Each role needs well under 128 VGPRs, so two
// workgroups (16 waves) fit a CU and the two halves of every SIMD pair overlap load latency,
// row arithmetic, column arithmetic and the output stream.
template <int L, int NLEV, int R, int TH, int NH, int MINW, typename InT, int LAYOUT, bool BF16>
__global__ __launch_bounds__(2 * NH, MINW) void k_swt_slide(const InT *__restrict__ in, void *__restrict__ out,
                                                            SlideGeom g, Taps<L> taps)
{
    using OutT = typename std::conditional<BF16, __hip_bfloat16, float>::type;
    const int P = g.P, W = g.W, H = g.H;
    const uint32_t band = (uint32_t)H * W;
    const ChunkRing<TH, 2> ring(P, H + VStep<L, NLEV, TH>::HALO);
    const PlaneSchedule sched(g);
    const bool is_h = threadIdx.x >= NH;                  // wave-uniform role
    const int t = is_h ? threadIdx.x - NH : threadIdx.x;
    if (is_h) {
        // a finished row -> LDS.  The row layout is permuted and the planes interleaved so that consecutive lanes (= consecutive
        // runs j) write consecutive 16-byte slots: column x = j*R + 2*q2 + e holds (lo, hi) at floats q2*(4*nrun) + 4*j + 2*e
#define WV_STAGE_PAIRS(PROW, CASC, w) do { \
            float *prow = PROW; \
            const int qstride = 4 * g.nrun; \
            _Pragma("unroll") \
            for (int q2 = 0; q2 < R / 2; ++q2) { \
                float4 v4; \
                v4.x = CASC::last(w, taps.lo, 2 * q2 + 0); v4.y = CASC::last(w, taps.hi, 2 * q2 + 0); \
                v4.z = CASC::last(w, taps.lo, 2 * q2 + 1); v4.w = CASC::last(w, taps.hi, 2 * q2 + 1); \
                *reinterpret_cast<float4 *>(prow + q2 * qstride) = v4; \
            } \
        } while (0)
        WV_SLIDE_PRODUCER(taps.lo, WV_STAGE_PAIRS);
#undef WV_STAGE_PAIRS
    } else {
        // ------------------------------------------------------------------ consumer: pass V
        const bool active = t < W;
        __builtin_amdgcn_s_setprio(kConsumerPrio);   // the critical role issues first
        const int tp = ((t % R) / 2) * (4 * g.nrun) + (t / R) * 4 + 2 * (t & 1);   // this column's (lo, hi) slot in the LDS row
        using VS = VStep<L, NLEV, TH>;
        SWT_STAMP_ROLE;
        for (int q = sched.first; q < sched.nq; q += sched.step) {
            OutT *oplane = reinterpret_cast<OutT *>(out) + (size_t)sched.at(q).plane * g.pstride;
            f32x2 tail[VS::HALO];
#pragma unroll
            for (int i = 0; i < VS::HALO; ++i) tail[i] = f32x2{0.f, 0.f};
            __syncthreads();       // chunk 0 produced
            for (int k = 0; k < ring.nchunks; ++k) {
                const int y0 = k * TH - VS::HALO;          // first output row this chunk emits (uniform)
                SWT_STAMP_START;
                if (active) {
                    const float *col = ring.buffer(k) + tp;
                    f32x2 cur[TH];
#pragma unroll
                    for (int i = 0; i < TH; ++i) cur[i] = *reinterpret_cast<const f32x2 *>(col + i * ring.pitch());
                    VS::template lower<1>(cur, tail, taps.lo);
                    SWT_STAMP(0);
                    if (y0 + TH <= 0) {                    // nothing to emit yet: only advance the state
                        VS::prime_last(cur, tail);
                    } else {
                        // byte offset of this lane inside an output row (< 2^32, host check); the four band rows are
                        // wave-uniform pointers (SGPR pairs, scalar adds): the band stride may exceed 32 bits in the
                        // band-major layout
                        const uint32_t o0 = (uint32_t)t * (uint32_t)sizeof(OutT);
                        const size_t bs = g.bstride;
                        VS::last(cur, tail, taps.lo, taps.hi, [&](int i, f32x2 a, f32x2 d) {
                            const int y = y0 + i;
                            if (y >= 0 && y < H) {
                                OutT *orow = oplane + (size_t)y * W;   // uniform: lives in an SGPR pair
                                store_row(orow, o0, (OutT)a.x);             // cA  = (row lo, col lo)
                                store_row(orow + bs, o0, (OutT)d.x);        // cH  = (row lo, col hi)
                                store_row(orow + 2 * bs, o0, (OutT)a.y);    // cV  = (row hi, col lo)
                                store_row(orow + 3 * bs, o0, (OutT)d.y);    // cD  = (row hi, col hi)
                            }
                        });
                    }
                }
                SWT_STAMP(1);
                __syncthreads();   // buffer k & 1 drained, buffer (k+1) & 1 full
                SWT_STAMP(2);
            }
        }
        SWT_STAMP_FLUSH(0);
    }
}

// Round 3, measured and removed: pulling a workgroup's NEXT plane into L2 in one burst at the start of each plane (one dword per
// 128-byte line, so that HBM sees one 50 KB read per plane instead of fifteen 3.5 KB reads mixed into the write stream):
// 1.126-1.130 ms against 1.062 ms back to back (the write stream evicts the lines before they are used: the reads happen
// twice).  LDS ring pitch W + {0, 4, 8, 12, 28}: no difference (profiles/r03_swt_experiments.txt).
// Decoupled roles were built and measured in round 2 (per-stage LDS ready / free counters instead of the chunk barrier:
// 4 stages x 8 rows with producer wave pairs alternating stages, and 2 stages x 16 rows with the stage released as soon as
// the consumers hold its rows in registers): bit-identical output, 1.22 ms and 1.16 ms against 1.08 ms for this kernel
// (2048 images, back to back) -- polling waves and the shorter per-stage batches cost more than the barrier wait they
// remove, which the second workgroup of the CU was already filling.  Removed; see DESIGN.md section 5.

bool slide_fits(const SwtShape &s, char *why, size_t why_len)
{
#define WV_NO(...) do { if (why) snprintf(why, why_len, __VA_ARGS__); return false; } while (0)
    if (!swt_config(s.L, s.level))
        WV_NO("%d taps at level %d (instantiated: 2 or 4 taps at levels 1-3, 8 or 10 taps at level 1)", s.L, s.level);
    if (s.in_layout != WV_LAYOUT_NCHW && !(s.in_layout == WV_LAYOUT_NHWC && s.C == 3))
        WV_NO("input layout %d with C = %d (NCHW, or NHWC with C == 3)", s.in_layout, s.C);
    const int halo = (s.L - 1) * ((1 << s.level) - 1);
    const int wmin = std::max(40, kSlideR + halo), hmin = std::max(40, kSlideTH + 2 * halo);
    if (s.W % 4 || s.W < wmin || s.W > kSlideNT) WV_NO("W = %d (W %% 4 == 0, %d <= W <= %d)", s.W, wmin, kSlideNT);
    if (s.H < hmin) WV_NO("H = %d (H >= %d)", s.H, hmin);
    const SlideRing r = slide_ring(s.W);
    if (kSlideTH * r.nrun > kSlideNT || r.lds > (size_t)kMaxLdsBytes - 2048)
        WV_NO("W = %d (LDS ring of %zu bytes for %d runs)", s.W, r.lds, r.nrun);
    if ((uint64_t)s.H * s.W * 4 >= (1ull << 30)) WV_NO("H*W = %lld (4*H*W < 2^30)", (long long)s.H * s.W);
    return true;
#undef WV_NO
}

// The CU count both sliding kernels size their persistent grids by: of the device that is current at the first sliding launch
// of the process.  A later launch on a device with another CU count gets that grid: correct (any grid is), not the intended size.
int slide_num_cu()
{
    static int num_cu = 0;
    if (!num_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        num_cu = prop.multiProcessorCount;
    }
    return num_cu;
}

template <int L, int NLEV>
static int launch_slide(const SwtShape &s, const void *in, void *out, const SlideGeom &g, size_t lds, const float *lo,
                        const float *hi, hipStream_t st)
{
    Taps<L> taps;
    for (int i = 0; i < L; ++i) { taps.lo[i] = lo[i]; taps.hi[i] = hi[i]; }
    return slide_io_dispatch(s, [&](auto in_t, auto layout, auto bf16) {
        using InT = decltype(in_t);
        return slide_launch<InT, layout()>(k_swt_slide<L, NLEV, kSlideR, kSlideTH, kSlideNT, kSlideMinW, InT, layout(), bf16()>,
                                           "k_swt_slide", "swt slide", kSlideMinW, in, out, g, lds, taps, st);
    });
}

int swt_slide_launch(const SwtShape &s, const void *in, void *out, const float *lo, const float *hi, hipStream_t st,
                     int out_layout, int64_t band_stride)
{
    const SlideRing r = slide_ring(s.W);
    SlideGeom g{};
    g.B = s.B; g.C = s.C; g.H = s.H; g.W = s.W;
    g.nrun = r.nrun; g.P = r.P;
    const size_t hw = (size_t)s.H * s.W;
    if (out_layout == WV_BANDS_OUTER) { g.pstride = hw; g.bstride = (size_t)band_stride; }
    else { g.pstride = 4 * hw; g.bstride = hw; }
#define WV_CFG(LL, NN) if (s.L == LL && s.level == NN) return launch_slide<LL, NN>(s, in, out, g, r.lds, lo, hi, st);
    WV_SWT_CONFIGS(WV_CFG)
#undef WV_CFG
    WV_FAIL(WV_ENOTSUP, "swt slide: %d taps at level %d", s.L, s.level);   // unreachable after slide_fits()
}

}  // namespace wv

#ifdef WV_SWT_STAMPS
// diagnostic build only: read and reset the cycle sums ([2 roles][8]; n <= 16 values)
extern "C" int wv_debug_swt_stamps(unsigned long long *host, int n)
{
    if (n < 0 || n > 16) return -1;
    const unsigned long long zero[16] = {0};
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(wv::g_swt_stamps), n * sizeof(unsigned long long)) != hipSuccess) return -5;
    if (hipMemcpyToSymbol(HIP_SYMBOL(wv::g_swt_stamps), zero, sizeof(zero)) != hipSuccess) return -5;
    return 0;
}
#endif
