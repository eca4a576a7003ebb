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
#include "swt.hpp"
#include <type_traits>
#include <vector>

namespace wv {

struct SlideGeom {
    int B, C, H, W;
    int P;          // ring pitch in floats
    int nrun;       // runs per row = ceil(W / R)
    int in_layout;
    int out_bf16;
    int coal;       // planar uint8, W % 16 == 0: producers load every pixel once, coalesced (see the producer role)
    int nxcd;       // 8: workgroups w, w+8, ... (one XCD, hardware round-robin) share images; 1: plain striding
    // output addressing in elements: plane (b, c) starts at (b*C + c) * pstride, its band k at + k * bstride.
    //   [B][C][4][H][W] (reference layout):  pstride = 4*H*W, bstride = H*W
    //   [4][B][C][H][W] (band-major, each band one contiguous NCHW batch):  pstride = H*W, bstride = B*C*H*W
    size_t pstride, bstride;
    unsigned long long *stamps;   // diagnostic build only
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
// STAMP = true is a diagnostic build (WV_SWT_STAMPS=1): per-wave s_memtime totals of the three segments of
// each role go to g.stamps (never read by the kernel, never part of an output).
#define WV_STAMP(var) do { if constexpr (STAMP) { __builtin_amdgcn_sched_barrier(0); var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); } } while (0)
template <int L, int NLEV, int R, int TH, int NH, int MINW, typename InT, int LAYOUT, bool BF16, bool STAMP = false>
__global__ __launch_bounds__(2 * NH, MINW) void k_swt_slide(const InT *__restrict__ in, void *__restrict__ out,
                                                            SlideGeom g, Taps<L> taps)
{
    uint64_t st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0, st5 = 0, acc_a = 0, acc_b = 0, acc_c = 0, acc_d = 0, acc_e = 0;
    using CH = Cascade<L, NLEV, R>;
    using Raw = SRaw<InT, LAYOUT>;
    using OutT = typename std::conditional<BF16, __hip_bfloat16, float>::type;
    constexpr int HALO = CH::HALO;
    constexpr int HB = (L / 2 - 1) * ((1 << NLEV) - 1);
    constexpr int HBa = (HB + 3) / 4 * 4;
    constexpr int NG = (HBa - HB + CH::NIN + 3) / 4;      // 4-pixel groups one run loads
    static_assert(R % 4 == 0, "run length must be a multiple of 4");
    extern __shared__ float4 ring4[];
    float *ring = reinterpret_cast<float *>(ring4);       // [2 buffers][2 planes][TH][P]
    const int P = g.P, W = g.W, H = g.H;
    const int buf_sz = 2 * TH * P;
    const int nchunks = (H + HALO + TH - 1) / TH;         // the cascade consumes H + HALO rows per plane
    const uint32_t band = (uint32_t)H * W;
    // Plane schedule.  Workgroup w runs on XCD w % 8 (round-robin dispatch) and every XCD has its own L2, so
    // the C channel planes of one interleaved (NHWC) image -- which all read the same bytes -- go to
    // neighbouring workgroups of ONE XCD: image b belongs to XCD b % nxcd, and the planes of an XCD's images
    // are dealt to its workgroups in (image, channel) order.  Two of the three reads then hit that L2.
    const int xcd = blockIdx.x % g.nxcd, wg_in_xcd = blockIdx.x / g.nxcd, wgs_per_xcd = gridDim.x / g.nxcd;
    const int nq = g.B > xcd ? (g.B - xcd + g.nxcd - 1) / g.nxcd * g.C : 0;   // planes this XCD owns
    const bool is_h = threadIdx.x >= NH;                  // wave-uniform role
    const int t = is_h ? threadIdx.x - NH : threadIdx.x;
    if (is_h) {
        // ------------------------------------------------------------------ producer: pass H
        // (row, run) of this producer thread.  Coalesced mode (planar uint8, W % 16 == 0) keeps the runs of one row
        // inside one wave -- 64 / nrun rows per wave -- so that neighbouring runs can hand over their pixels with
        // ds_bpermute: each thread then issues ONE 16-byte load per chunk and every input byte is read exactly once
        // (the strided form touches each cache line of its 40-pixel window ten times).
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
            // end of a chunk: buffer k & 1 is full; buffer (k+1) & 1 was drained before this barrier
            auto hand_over = [&]() {
                WV_STAMP(st2);
                __syncthreads();
                WV_STAMP(st3);
                if constexpr (STAMP) { acc_a += st1 - st0; acc_b += st2 - st5; acc_c += st3 - st2; acc_d += st4 - st1; acc_e += st5 - st4; }
            };
            // The two fetch modes have a chunk loop each: neither holds the other's addresses in registers, and the wait
            // for the strided loads in front of the conversion does not also wait for the coalesced row just issued.
            if (coal) {
                if constexpr (CAN_COAL) {
                    issue_row(0);
                    for (int k = 0; k < nchunks; ++k) {
                        WV_STAMP(st0);
                        // Every pixel is converted once and every level value computed once per row: run j owns
                        // outputs 0 .. R-1 of each level and its right neighbour hands over the rest (RunCascade).
                        // All of it feeds ds_bpermute, so it runs in every lane of the wave -- spare lanes hold a
                        // valid row -- and only the LDS write is per lane.  A wave whose rows all lie past the
                        // TH rows of the chunk or past the H + HALO rows the column cascade consumes skips the chunk.
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
                            WV_STAMP(st1);
                            if (k + 1 < nchunks) issue_row(k + 1);             // flies during this chunk's arithmetic
                            WV_STAMP(st4);
                            RC::template lower<1>(w, taps.lo, lane_right);
                            WV_STAMP(st5);
                            if (active && k * TH + rr < H + HALO) {
                                float *prow = ring + (k & 1) * buf_sz + rr * (2 * P) + 4 * j;   // row layout: see the strided loop
                                const int qstride = 4 * g.nrun;
#pragma unroll
                                for (int q2 = 0; q2 < R / 2; ++q2) {
                                    float4 v4;
                                    v4.x = RC::last(w, taps.lo, 2 * q2 + 0); v4.y = RC::last(w, taps.hi, 2 * q2 + 0);
                                    v4.z = RC::last(w, taps.lo, 2 * q2 + 1); v4.w = RC::last(w, taps.hi, 2 * q2 + 1);
                                    *reinterpret_cast<float4 *>(prow + q2 * qstride) = v4;
                                }
                            }
                        } else {
                            if (k + 1 < nchunks) issue_row(k + 1);
                            if constexpr (STAMP) st1 = st4 = st5 = st0;
                        }
                        hand_over();
                    }
                }
            } else {
                if (active) fetch(0);
                for (int k = 0; k < nchunks; ++k) {
                    WV_STAMP(st0);
                    if (active) {
                        float v[NG * 4];
#pragma unroll
                        for (int q = 0; q < NG; ++q) {
                            const float4 p4 = s_convert4<InT, LAYOUT>(raw[q], c);
                            v[4 * q + 0] = p4.x; v[4 * q + 1] = p4.y; v[4 * q + 2] = p4.z; v[4 * q + 3] = p4.w;
                        }
                        WV_STAMP(st1);
                        if (k + 1 < nchunks) fetch(k + 1);              // next chunk's pixels fly during the arithmetic
                        WV_STAMP(st4);
                        // in-place cascade on v[off ..): element i of the run lives at v[i + off]
                        constexpr int off = HBa - HB;
                        float w[CH::NIN];
#pragma unroll
                        for (int i = 0; i < CH::NIN; ++i) w[i] = v[i + off];
                        CH::template lower<1>(w, taps.lo);
                        WV_STAMP(st5);
                        // LDS row layout is permuted and the planes interleaved so that consecutive lanes (= consecutive
                        // runs j) write consecutive 16-byte slots: column x = j*R + 2*q2 + e holds (lo, hi) at floats
                        // q2*(4*nrun) + 4*j + 2*e of its row
                        float *prow = ring + (k & 1) * buf_sz + rr * (2 * P) + 4 * j;
                        const int qstride = 4 * g.nrun;
#pragma unroll
                        for (int q2 = 0; q2 < R / 2; ++q2) {
                            float4 v4;
                            v4.x = CH::last(w, taps.lo, 2 * q2 + 0); v4.y = CH::last(w, taps.hi, 2 * q2 + 0);
                            v4.z = CH::last(w, taps.lo, 2 * q2 + 1); v4.w = CH::last(w, taps.hi, 2 * q2 + 1);
                            *reinterpret_cast<float4 *>(prow + q2 * qstride) = v4;
                        }
                    }
                    hand_over();
                }
            }
            __syncthreads();       // pairs with the consumer's last barrier of the plane
        }
    } else {
        // ------------------------------------------------------------------ consumer: pass V
        const bool active = t < W;
        __builtin_amdgcn_s_setprio(kConsumerPrio);   // the critical role issues first
        // this column's (lo, hi) slot in the permuted LDS row (see pass H)
        const int tp = ((t % R) / 2) * (4 * g.nrun) + (t / R) * 4 + 2 * (t & 1);
        using VS = VStep<L, NLEV, TH>;
        for (int q = wg_in_xcd; q < nq; q += wgs_per_xcd) {
            const int m = q / g.C, pc = (xcd + g.nxcd * m) * g.C + (q - m * g.C);
            OutT *oplane = reinterpret_cast<OutT *>(out) + (size_t)pc * g.pstride;
            f32x2 tail[HALO];
#pragma unroll
            for (int i = 0; i < HALO; ++i) tail[i] = f32x2{0.f, 0.f};
            __syncthreads();       // chunk 0 produced
            for (int k = 0; k < nchunks; ++k) {
                const int y0 = k * TH - HALO;              // first output row this chunk emits (uniform)
                WV_STAMP(st0);
                if (active) {
                    const float *col = ring + (k & 1) * buf_sz + tp;
                    f32x2 cur[TH];
#pragma unroll
                    for (int i = 0; i < TH; ++i) cur[i] = *reinterpret_cast<const f32x2 *>(col + i * (2 * P));
                    VS::template lower<1>(cur, tail, taps.lo);
                    WV_STAMP(st1);
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
                WV_STAMP(st2);
                __syncthreads();   // buffer k & 1 drained, buffer (k+1) & 1 full
                WV_STAMP(st3);
                if constexpr (STAMP) { acc_a += st1 - st0; acc_b += st2 - st1; acc_c += st3 - st2; }
            }
        }
    }
    if constexpr (STAMP) {
        if ((threadIdx.x & 63) == 0) {
            unsigned long long *o = g.stamps + ((size_t)blockIdx.x * (2 * NH / 64) + threadIdx.x / 64) * 8;
            o[0] = acc_a; o[1] = acc_b; o[2] = acc_c; o[3] = is_h; o[4] = acc_d; o[5] = acc_e;
        }
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

// (taps, levels) with a sliding instantiation (swt_slide_launch): the shipped configs (haar L1 = c0, db2 L3 = c1), the other
// levels of the 2- and 4-tap wavelets, and level 1 of the 8- and 10-tap wavelets the studies sweep (db4, bior4.4).
static bool slide_config(int L, int n)
{
    return ((L == 2 || L == 4) && n >= 1 && n <= 3) || ((L == 8 || L == 10) && n == 1);
}

bool slide_fits(const SwtShape &s, char *why, size_t why_len)
{
#define WV_NO(...) do { if (why) snprintf(why, why_len, __VA_ARGS__); return false; } while (0)
    if (!slide_config(s.L, s.level))
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

// Diagnostic build (WV_SWT_STAMPS=1): run the STAMP instantiation once, synchronously, and print where each role's
// cycles go.
template <typename Kern, typename InT, int L>
static int run_stamped(Kern kstamp, int64_t grid, size_t lds, hipStream_t st, const InT *in, void *out, SlideGeom g,
                       const Taps<L> &taps)
{
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kstamp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const size_t nw = (size_t)grid * (2 * kSlideNT / 64);
    unsigned long long *dbuf = nullptr;
    if (hipMalloc(&dbuf, nw * 8 * sizeof(unsigned long long)) != hipSuccess) WV_FAIL(WV_EHIP, "stamps: hipMalloc");
    g.stamps = dbuf;
    hipLaunchKernelGGL(kstamp, dim3((unsigned)grid), dim3(2 * kSlideNT), lds, st, in, out, g, taps);
    std::vector<unsigned long long> hbuf(nw * 8, 0);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(hbuf.data(), dbuf, nw * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(dbuf);
    double a[2][6] = {{0}, {0}};
    size_t cnt[2] = {0, 0};
    for (size_t i = 0; i < nw; ++i) {
        const int role = (int)hbuf[8 * i + 3];
        for (int c = 0; c < 6; ++c) a[role][c] += (double)hbuf[8 * i + c];
        cnt[role]++;
    }
    fprintf(stderr, "[swt stamps] V waves=%zu: LDS read+lower(pl0) %.0f | rest(last+stores, pl1) %.0f | barrier %.0f\n", cnt[0],
            a[0][0] / cnt[0], a[0][1] / cnt[0], a[0][2] / cnt[0]);
    fprintf(stderr, "[swt stamps] H waves=%zu: wait loads+convert %.0f | issue next loads %.0f | lower levels %.0f | last level+LDS write %.0f | barrier %.0f\n",
            cnt[1], a[1][0] / cnt[1], a[1][4] / cnt[1], a[1][5] / cnt[1], a[1][1] / cnt[1], a[1][2] / cnt[1]);
    return WV_OK;
}

template <int L, int NLEV, typename InT, int LAYOUT, bool BF16>
static int launch_slide(const void *in, void *out, SlideGeom g, size_t lds, const Taps<L> &taps, hipStream_t st)
{
    constexpr int R = kSlideR, TH = kSlideTH, NT = kSlideNT, MINW = kSlideMinW;
    auto kern = k_swt_slide<L, NLEV, R, TH, NT, MINW, InT, LAYOUT, BF16>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) WV_FAIL(WV_EHIP, "swt slide: hipFuncSetAttribute(%zu): %s", lds, hipGetErrorString(e));
    }
    static int num_cu = 0;
    if (!num_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
            WV_FAIL(WV_EHIP, "swt slide: device query failed");
        num_cu = prop.multiProcessorCount;
    }
    const int by_lds = std::max<int>(1, (int)((size_t)kMaxLdsBytes / (lds + 512)));
    const int per_cu = std::min(by_lds, std::max(1, MINW * 256 / (2 * NT)));
    const int64_t planes = (int64_t)g.B * g.C;
    int64_t grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    g.coal = std::is_same<InT, uint8_t>::value && LAYOUT == 0 && R == 16 && g.W % 16 == 0 && g.nrun <= 16 &&
             (int64_t)g.H * g.W % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    g.nxcd = kXcds;
    if (grid < planes) grid -= grid % g.nxcd;      // persistent launch: same number of workgroups on every XCD
    if (grid <= 0 || grid % g.nxcd) g.nxcd = 1, grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    if constexpr ((L == 4 && NLEV == 3) || (L == 2 && NLEV == 1))   // the two shipped configs have a STAMP build
        if (::wv::tune("WV_SWT_STAMPS"))
            return run_stamped(k_swt_slide<L, NLEV, R, TH, NT, MINW, InT, LAYOUT, BF16, true>, grid, lds, st,
                               (const InT *)in, out, g, taps);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(2 * NT), lds, st, (const InT *)in, out, g, taps);
    WV_CHECK_LAUNCH("k_swt_slide");
    return WV_OK;
}

template <int L, int NLEV>
static int slide_types(const SwtShape &s, const void *in, void *out, const SlideGeom &g, size_t lds, const float *lo,
                       const float *hi, hipStream_t st)
{
    Taps<L> taps;
    for (int i = 0; i < L; ++i) { taps.lo[i] = lo[i]; taps.hi[i] = hi[i]; }
    const bool nhwc3 = s.in_layout == WV_LAYOUT_NHWC;   // C == 3 (slide_fits)
#define WV_GO(T, LAY, BF) return launch_slide<L, NLEV, T, LAY, BF>(in, out, g, lds, taps, st)
    if (s.in_dtype == WV_DT_U8) {
        if (nhwc3) { if (g.out_bf16) WV_GO(uint8_t, 1, true); WV_GO(uint8_t, 1, false); }
        if (g.out_bf16) WV_GO(uint8_t, 0, true);
        WV_GO(uint8_t, 0, false);
    }
    if (nhwc3) { if (g.out_bf16) WV_GO(float, 1, true); WV_GO(float, 1, false); }
    if (g.out_bf16) WV_GO(float, 0, true);
    WV_GO(float, 0, false);
#undef WV_GO
}

int swt_slide_launch(const SwtShape &s, const void *in, void *out, const float *lo, const float *hi, hipStream_t st,
                     int out_layout, int64_t band_stride)
{
    const SlideRing r = slide_ring(s.W);
    SlideGeom g{};
    g.B = s.B; g.C = s.C; g.H = s.H; g.W = s.W; g.in_layout = s.in_layout; g.out_bf16 = s.out_dtype == WV_DT_BF16;
    g.nrun = r.nrun; g.P = r.P;
    const size_t hw = (size_t)s.H * s.W;
    if (out_layout == WV_BANDS_OUTER) { g.pstride = hw; g.bstride = (size_t)band_stride; }
    else { g.pstride = 4 * hw; g.bstride = hw; }
#define WV_CFG(LL, NN) if (s.L == LL && s.level == NN) return slide_types<LL, NN>(s, in, out, g, r.lds, lo, hi, st)
    WV_CFG(4, 3); WV_CFG(2, 1);
    WV_CFG(4, 1); WV_CFG(4, 2); WV_CFG(2, 2); WV_CFG(2, 3); WV_CFG(8, 1); WV_CFG(10, 1);
#undef WV_CFG
    WV_FAIL(WV_ENOTSUP, "swt slide: %d taps at level %d", s.L, s.level);   // unreachable after slide_fits()
}

}  // namespace wv
