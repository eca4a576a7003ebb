// The sliding SWT scheme, once: what k_swt_slide (swt_slide.hip, four bands) and k_swt_band (swt_band.hip, one band) are
// made of; only those two include it.  A persistent workgroup of 2 * NT threads owns whole (image, channel) planes and
// walks down each TH rows at a time: producer waves row-filter the rows of chunk k+1 into one half of an LDS ring while
// consumer waves (thread = column) run the column cascade over chunk k from the other half; a barrier per chunk swaps them.
//   PlaneSchedule, ChunkRing   which planes a workgroup computes in which order; the ring and chunk count both roles walk
//   WV_SLIDE_PRODUCER          the producer role of a workgroup: both fetch modes, all levels along x, the barriers
//   VStep, store_row           what the consumer chunk loops of the two kernels are made of (the loops stay in the kernels)
//   slide_launch               the persistent launch rule;  slide_io_dispatch: the (dtype, layout, bf16) instantiation
// The producers differ in what a staged row holds -- interleaved (lo, hi) pairs or one filter's outputs -- which arrives
// as the kernel's stage and a pitch.  Nothing in this file asks which kernel it serves.
#pragma once
#include "swt.hpp"
#include <type_traits>

namespace wv {

// The one configuration every (taps, levels) instantiation uses: runs of R columns, TH rows per step, NT threads per
// role (W <= NT), MINW workgroups per CU.
constexpr int kSlideR = 16, kSlideTH = 16, kSlideNT = 256, kSlideMinW = 4;
constexpr int kPitchPad = 4;      // LDS ring pitch = nrun * R + 4 floats
// A/B on MI355X in one session, db2 level 3, 2048 images: consumer (column) waves at raised issue priority: 1.148 ms vs
// 1.19 ms at equal priority (they are the critical role)
constexpr int kConsumerPrio = 2;
constexpr int kXcds = 8;          // workgroup w runs on XCD w % 8 (hardware round-robin)

// Diagnostic build only (-DWV_SWT_STAMPS on swt_slide.hip, tools/build_variant.sh, tools/swt_stamps.py): cycles per segment
// of each role's chunk, summed in registers over the launch, then added by lane 0 of the wave to a device array that nothing
// else reads ([role][segment]).  SWT_STAMP_ROLE opens a role, _START a chunk; SWT_STAMP closes a segment; _FLUSH ends the role.
#ifdef WV_SWT_STAMPS
__device__ unsigned long long g_swt_stamps[16];
#define SWT_STAMP_NOW(var) do { __builtin_amdgcn_sched_barrier(0); var = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); } while (0)
#define SWT_STAMP_ROLE unsigned long long stamp_ = 0, acc_[5] = {0, 0, 0, 0, 0}
#define SWT_STAMP_START SWT_STAMP_NOW(stamp_)
#define SWT_STAMP(seg) do { unsigned long long now_; SWT_STAMP_NOW(now_); acc_[seg] += now_ - stamp_; stamp_ = now_; } while (0)
#define SWT_STAMP_FLUSH(role) do { if ((threadIdx.x & 63) == 0) for (int i_ = 0; i_ < 5; ++i_) \
    atomicAdd(&g_swt_stamps[(role) * 8 + i_], acc_[i_]); } while (0)
#else
#define SWT_STAMP_ROLE do { } while (0)
#define SWT_STAMP_START do { } while (0)
#define SWT_STAMP(seg) do { } while (0)
#define SWT_STAMP_FLUSH(role) do { } while (0)
#endif

// Each kernel keeps its own geometry argument (SlideGeom in swt_slide.hip, BandGeom in swt_band.hip), laid out as it was:
// any other layout of the argument block moves the scalar loads and with them s_waitcnt counts and SGPR spills in 24-32
// of the 64 four-band kernels (profiles/swt_slide_refactor.txt, section 1).  The shared code reads these int members of
// either: B, C, H, W; P, the ring pitch in floats; nrun, runs per row = ceil(W / R); coal, planar uint8 and W % 16 == 0:
// producers load every pixel once, coalesced (see WV_SLIDE_PRODUCER); nxcd, 8: workgroups w, w+8, ... (one XCD, hardware
// round-robin) share images, 1: plain striding.

// Plane schedule.  Workgroup w runs on XCD w % 8 (round-robin dispatch) and every XCD has its own L2, so
// the C channel planes of one interleaved (NHWC) image -- which all read the same bytes -- go to
// neighbouring workgroups of ONE XCD: image b belongs to XCD b % nxcd, and the planes of an XCD's images
// are dealt to its workgroups in (image, channel) order.  Two of the three reads then hit that L2.
struct PlaneSchedule {
    struct Plane { int b, c, plane; };   // plane = b * C + c
    int xcd, nxcd, C;
    int first, step, nq;                 // this workgroup's slots among the nq planes its XCD owns
    template <typename Geom>
    __device__ __forceinline__ explicit PlaneSchedule(const Geom &g)
        : xcd(blockIdx.x % g.nxcd), nxcd(g.nxcd), C(g.C), first(blockIdx.x / g.nxcd), step(gridDim.x / g.nxcd),
          nq(g.B > xcd ? (g.B - xcd + g.nxcd - 1) / g.nxcd * g.C : 0) {}
    __device__ __forceinline__ Plane at(int q) const
    {
        const int m = q / C, c = q - m * C, b = xcd + nxcd * m;
        return {b, c, b * C + c};
    }
};

// The LDS ring as both roles walk it: two buffers of TH staged rows, NPL row-filtered planes of pitch P per row; chunk k
// lives in buffer k & 1 and a plane takes nchunks chunks for the `rows` = H + HALO rows the cascade consumes.  Built once per
// workgroup, before the roles part.  The array is named here, not handed over, so that addresses start from a known LDS base.
extern __shared__ float4 slide_ring4[];
template <int TH, int NPL>
struct ChunkRing {
    int P, buf_sz, nchunks;
    __device__ __forceinline__ ChunkRing(int P_, int rows) : P(P_), buf_sz(NPL * TH * P_), nchunks((rows + TH - 1) / TH) {}
    __device__ __forceinline__ float *buffer(int k) const { return reinterpret_cast<float *>(slide_ring4) + (k & 1) * buf_sz; }
    __device__ __forceinline__ int pitch() const { return NPL * P; }
};

// Streaming form of the cascade for pass V: a thread keeps, per column, the last (L-1)*2^(l-1)
// inputs of every level l in registers ("tails", HALO values in all), so each step costs exactly
// L MACs per level per new row -- no halo recompute -- and emits outputs delayed by HALO rows.
// The arithmetic per output is identical to Cascade (same taps, same order).
// The four-band kernel runs it on (row-lo, row-hi) PAIRS: the two row-filtered planes go through identical arithmetic,
// so the consumer keeps them as 2-vectors and every multiply-add becomes one v_pk_fma_f32 -- half the instructions a
// wave has to issue for the same (bitwise identical) result.  The LDS ring holds the planes interleaved.
using f32x2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2 fma_s(float s, f32x2 x, f32x2 a)
{
    const f32x2 sv = {s, s};
    return __builtin_elementwise_fma(sv, x, a);
}
__device__ __forceinline__ float fma_s(float s, float x, float a) { return fmaf(s, x, a); }

// The single-band kernel runs the same cascade on one plane: V = float, last1() for its one column filter.
template <int L, int NLEV, int N, typename V = f32x2>
struct VStep {
    using T = V;
    static constexpr int HALO = (L - 1) * ((1 << NLEV) - 1);
    // level LEV reads its inputs at stride S and keeps TT of them, at tail[OFF ..)
    template <int LEV>
    struct Lv {
        static constexpr int S = 1 << (LEV - 1), TT = (L - 1) * S, OFF = (L - 1) * (S - 1);
    };
    // levels LEV .. NLEV-1: cur[] holds N new level-LEV inputs on entry, N new level-NLEV inputs on exit
    template <int LEV>
    static __device__ __forceinline__ void lower(T (&cur)[N], T (&tail)[HALO], const float (&lo)[L])
    {
        if constexpr (LEV < NLEV) {
            constexpr int S = Lv<LEV>::S;
            T seq[Lv<LEV>::TT + N];
            join<LEV>(seq, tail, cur);
#pragma unroll
            for (int t = 0; t < N; ++t) {
                T a = lo[0] * seq[t + S * (L - 1)];
#pragma unroll
                for (int m = 1; m < L; ++m) a = fma_s(lo[m], seq[t + S * (L - 1 - m)], a);
                cur[t] = a;
            }
            keep<LEV>(tail, seq);
            lower<LEV + 1>(cur, tail, lo);
        }
    }
    // last level: seq = tail ++ cur; out(t) for t < N; tail updated
    template <typename Emit>
    static __device__ __forceinline__ void last(const T (&cur)[N], T (&tail)[HALO], const float (&lo)[L],
                                                const float (&hi)[L], Emit emit)
    {
        constexpr int S = Lv<NLEV>::S;
        T seq[Lv<NLEV>::TT + N];
        join<NLEV>(seq, tail, cur);
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
        keep<NLEV>(tail, seq);
    }
    // last level of one band: the one column filter f, same taps in the same order
    template <typename Emit>
    static __device__ __forceinline__ void last1(const T (&cur)[N], T (&tail)[HALO], const float (&f)[L], Emit emit)
    {
        constexpr int S = Lv<NLEV>::S;
        T seq[Lv<NLEV>::TT + N];
        join<NLEV>(seq, tail, cur);
#pragma unroll
        for (int t = 0; t < N; ++t) {
            T a = f[0] * seq[t + S * (L - 1)];
#pragma unroll
            for (int m = 1; m < L; ++m) a = fma_s(f[m], seq[t + S * (L - 1 - m)], a);
            emit(t, a);
        }
        keep<NLEV>(tail, seq);
    }
    // warm-up: only refresh the last level's tail
    static __device__ __forceinline__ void prime_last(const T (&cur)[N], T (&tail)[HALO])
    {
        T seq[Lv<NLEV>::TT + N];
        join<NLEV>(seq, tail, cur);
        keep<NLEV>(tail, seq);
    }

private:
    // seq = level LEV's tail ++ its N new inputs
    template <int LEV>
    static __device__ __forceinline__ void join(T (&seq)[Lv<LEV>::TT + N], const T (&tail)[HALO], const T (&cur)[N])
    {
#pragma unroll
        for (int i = 0; i < Lv<LEV>::TT; ++i) seq[i] = tail[Lv<LEV>::OFF + i];
#pragma unroll
        for (int i = 0; i < N; ++i) seq[Lv<LEV>::TT + i] = cur[i];
    }
    // the last TT inputs of seq are level LEV's tail for the next step
    template <int LEV>
    static __device__ __forceinline__ void keep(T (&tail)[HALO], const T (&seq)[Lv<LEV>::TT + N])
    {
#pragma unroll
        for (int i = 0; i < Lv<LEV>::TT; ++i) tail[Lv<LEV>::OFF + i] = seq[N + i];
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

// ------------------------------------------------------------------------------- producer role: pass H
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

// The producer role of a workgroup, all its planes, as TEXT: thread t of the role fetches the TH input rows of every chunk,
// filters them along x in registers (levels below the last with the approximation taps LO) and stages the last level into
// ring buffer k & 1.  A finished live row is written by STAGE(prow, CASC, w), a macro of the kernel's: prow is the row's first
// slot of run j (run j owns floats 4*j .. 4*j+3 of every 4*nrun-float group of the row) and CASC::last(w, f, i) is level-NLEV
// output i of the run under filter f.  Barriers: one per chunk and one that pairs with the consumer's last of the plane.
// A macro, not a function: as a __forceinline__ function template every kernel compiled to other code than the hand-inlined
// text, the consumer half included (profiles/swt_slide_refactor.txt, section 1).  It expands inside a kernel template over
// <L, NLEV, R, TH, InT, LAYOUT> and reads in (the batch), H, W, band (= H * W, uint32_t), t, sched, ring and g (the geometry).
//   lane set-up   (row, run) of this producer thread.  Coalesced mode (planar uint8, W % 16 == 0) keeps the runs of one row
//                 inside one wave -- 64 / nrun rows per wave -- so that neighbouring runs can hand over their pixels with
//                 ds_bpermute (lane_left / lane_right are lane byte addresses; periodic: the row wraps onto itself): each
//                 thread then issues ONE 16-byte load per chunk and every input byte is read exactly once (the strided form
//                 touches each cache line of its 40-pixel window ten times).  Spare lanes load a valid row too.
//   fetch         strided mode: input row of virtual row v = chunk*TH + rr is y = v - HB (wrapped; rows past H + HA wrap too);
//                 issue_row, coalesced mode: every lane of the wave (the exchange reads all of them)
//   chunk loops   The two fetch modes have a chunk loop each: neither holds the other's addresses in registers, and the wait
//                 for the strided loads in front of the conversion does not also wait for the coalesced row just issued.
//                 The next chunk's pixels are requested before this chunk's arithmetic and fly during it.
//   coalesced     Every pixel is converted once and every level value computed once per row: run j owns outputs 0 .. R-1 of
//                 each level and its right neighbour hands over the rest (RunCascade).  All of it feeds ds_bpermute, so it
//                 runs in every lane of the wave and only the LDS write is per lane.  A wave whose rows all lie past the TH
//                 rows of the chunk or past the H + HALO rows the column cascade consumes skips the chunk.  The pixel window
//                 [16j - HBa, 16j - HBa + 4 NGC) is left neighbour | own | right neighbour; gpx is a constant after unrolling.
//   strided       in-place cascade on v[HBa - HB ..): element i of the run lives at v[i + HBa - HB].  The __syncthreads at
//                 the end of a chunk, either mode: buffer k & 1 is full; buffer (k+1) & 1 was drained before this barrier
#define WV_SLIDE_PRODUCER(LO, STAGE) do { \
    using CH = Cascade<L, NLEV, R>;                                                                                        \
    constexpr int HALO = CH::HALO;                                                                                         \
    constexpr int HB = (L / 2 - 1) * ((1 << NLEV) - 1);                                                                    \
    constexpr int HBa = (HB + 3) / 4 * 4;                                                                                  \
    constexpr int NG = (HBa - HB + CH::NIN + 3) / 4;      /* 4-pixel groups one run loads */                               \
    static_assert(R % 4 == 0, "run length must be a multiple of 4");                                                       \
    const int nchunks = ring.nchunks;                                                                                      \
    int rr = t / g.nrun, j = t - rr * g.nrun;                                                                              \
    bool active = t < TH * g.nrun;                                                                                         \
    int lane_left = 0, lane_right = 0, rr_ld = 0, wrow0 = 0;                                                               \
    if (g.coal) {                                                                                                          \
        const int l = t & 63, rpw = 64 / g.nrun, lr = l / g.nrun;                                                          \
        j = l - lr * g.nrun;                                                                                               \
        wrow0 = (t >> 6) * rpw;                                              /* first row of this wave */                  \
        rr = wrow0 + lr;                                                                                                   \
        active = lr < rpw && rr < TH;                                                                                      \
        rr_ld = min(rr, TH - 1);                                                                                           \
        lane_left = (lr * g.nrun + (j == 0 ? g.nrun - 1 : j - 1)) * 4;                                                     \
        lane_right = (lr * g.nrun + (j == g.nrun - 1 ? 0 : j + 1)) * 4;                                                    \
        if (lr >= rpw) lane_left = lane_right = 0;                                                                         \
    }                                                                                                                      \
    SWT_STAMP_ROLE;                                                                                                        \
    for (int q = sched.first; q < sched.nq; q += sched.step) {                                                             \
        const auto p = sched.at(q);                                                                                        \
        const int c = p.c;                                                                                                 \
        const InT *img = LAYOUT == 0 ? in + (size_t)p.plane * band : in + (size_t)p.b * band * 3;                          \
        SRaw<InT, LAYOUT> raw[NG];                                                                                         \
        auto fetch = [&](int chunk) {                                                                                      \
            int y = chunk * TH + rr - HB;                                                                                  \
            y = y >= H ? y - H : y;                                                                                        \
            const uint32_t row = (uint32_t)wrap_once(y, H) * (uint32_t)W;                                                  \
            const int gx0 = j * R - HBa;                                                                                   \
            _Pragma("unroll")                                                                                              \
            for (int k = 0; k < NG; ++k)                                                                                   \
                raw[k] = s_fetch4<InT, LAYOUT>(img, row + (uint32_t)wrap_once(gx0 + 4 * k, W), c);                         \
        };                                                                                                                 \
        constexpr bool CAN_COAL = sizeof(InT) == 1 && LAYOUT == 0 && R == 16 && NG * 4 - HBa <= 32;                        \
        uint32_t own[4] = {0, 0, 0, 0};                                                                                    \
        auto issue_row = [&](int chunk) {                                                                                  \
            int y = chunk * TH + rr_ld - HB;                                                                               \
            y = y >= H ? y - H : y;                                                                                        \
            const uint4 v4 = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(img) +                     \
                                                              (size_t)wrap_once(y, H) * W + j * R);                        \
            own[0] = v4.x; own[1] = v4.y; own[2] = v4.z; own[3] = v4.w;                                                    \
        };                                                                                                                 \
        const bool coal = CAN_COAL && g.coal;   /* uniform */                                                              \
        if (coal) {                                                                                                        \
            if constexpr (CAN_COAL) {                                                                                      \
                issue_row(0);                                                                                              \
                for (int k = 0; k < nchunks; ++k) {                                                                        \
                    SWT_STAMP_START;                                                                                       \
                    using RC = RunCascade<L, NLEV, R>;                                                                     \
                    constexpr int NGC = (HBa - HB + RC::NPIX + 3) / 4;     /* 4-pixel groups level 1 reads */              \
                    static_assert(HBa <= 16 && 4 * NGC - HBa <= 32, "the pixel window must end in the neighbouring runs"); \
                    const int wrow = __builtin_amdgcn_readfirstlane(wrow0);          /* wave-uniform */                    \
                    const bool live = wrow < TH && k * TH + wrow < H + HALO;                                               \
                    if (live) {                                                                                            \
                        float w[RC::NW], v[NGC * 4];                                                                       \
                        _Pragma("unroll")                                                                                  \
                        for (int kk = 0; kk < NGC; ++kk) {                                                                 \
                            const int gpx = 4 * kk - HBa;                                                                  \
                            uint32_t d;                                                                                    \
                            if (gpx < 0)                                                                                   \
                                d = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_left, (int)own[(gpx + 16) / 4]);           \
                            else if (gpx < 16)                                                                             \
                                d = own[gpx / 4];                                                                          \
                            else                                                                                           \
                                d = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_right, (int)own[(gpx - 16) / 4]);          \
                            const float4 p4 = u8x4_to_unit(d);                                                             \
                            v[4 * kk + 0] = p4.x; v[4 * kk + 1] = p4.y; v[4 * kk + 2] = p4.z; v[4 * kk + 3] = p4.w;        \
                        }                                                                                                  \
                        _Pragma("unroll")                                                                                  \
                        for (int i = 0; i < RC::NPIX; ++i) w[i] = v[i + HBa - HB];                                         \
                        SWT_STAMP(0);                                                                                      \
                        if (k + 1 < nchunks) issue_row(k + 1);                                                             \
                        SWT_STAMP(1);                                                                                      \
                        RC::template lower<1>(w, LO, lane_right);                                                          \
                        SWT_STAMP(2);                                                                                      \
                        if (active && k * TH + rr < H + HALO)                                                              \
                            STAGE(ring.buffer(k) + rr * ring.pitch() + 4 * j, RC, w);                                      \
                    } else {                                                                                               \
                        if (k + 1 < nchunks) issue_row(k + 1);                                                             \
                    }                                                                                                      \
                    SWT_STAMP(3);                                                                                          \
                    __syncthreads();                                                                                       \
                    SWT_STAMP(4);                                                                                          \
                }                                                                                                          \
            }                                                                                                              \
        } else {                                                                                                           \
            if (active) fetch(0);                                                                                          \
            for (int k = 0; k < nchunks; ++k) {                                                                            \
                SWT_STAMP_START;                                                                                           \
                if (active) {                                                                                              \
                    float v[NG * 4];                                                                                       \
                    _Pragma("unroll")                                                                                      \
                    for (int q = 0; q < NG; ++q) {                                                                         \
                        const float4 p4 = s_convert4<InT, LAYOUT>(raw[q], c);                                              \
                        v[4 * q + 0] = p4.x; v[4 * q + 1] = p4.y; v[4 * q + 2] = p4.z; v[4 * q + 3] = p4.w;                \
                    }                                                                                                      \
                    SWT_STAMP(0);                                                                                          \
                    if (k + 1 < nchunks) fetch(k + 1);                                                                     \
                    SWT_STAMP(1);                                                                                          \
                    float w[CH::NIN];                                                                                      \
                    _Pragma("unroll")                                                                                      \
                    for (int i = 0; i < CH::NIN; ++i) w[i] = v[i + HBa - HB];                                              \
                    CH::template lower<1>(w, LO);                                                                          \
                    SWT_STAMP(2);                                                                                          \
                    STAGE(ring.buffer(k) + rr * ring.pitch() + 4 * j, CH, w);                                              \
                }                                                                                                          \
                SWT_STAMP(3);                                                                                              \
                __syncthreads();                                                                                           \
                SWT_STAMP(4);                                                                                              \
            }                                                                                                              \
        }                                                                                                                  \
        __syncthreads();       /* pairs with the consumer's last barrier of the plane */                                   \
    }                                                                                                                      \
    SWT_STAMP_FLUSH(1);                                                                                                    \
} while (0)

// ------------------------------------------------------------------------------- host side
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

// Compute units of the device, asked once per process (swt_slide.hip); 0: the query failed.  Not exported.
__attribute__((visibility("hidden"))) int slide_num_cu();

// The persistent launch of a sliding kernel compiled for `minw` waves per SIMD: workgroups per CU by the LDS ring and by
// the compiled occupancy, one workgroup per plane at most, and the same number of workgroups on every XCD when a
// workgroup gets several planes (PlaneSchedule).  Fills g.coal and g.nxcd.  `name` labels a failed launch, `what` the other errors.
template <typename InT, int LAYOUT, typename Kern, typename Geom, typename TapsT>
static int slide_launch(Kern kern, const char *name, const char *what, int minw, const void *in, void *out, Geom g, size_t lds,
                        const TapsT &taps, hipStream_t st)
{
    constexpr int R = kSlideR, NT = kSlideNT;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) WV_FAIL(WV_EHIP, "%s: hipFuncSetAttribute(%zu): %s", what, lds, hipGetErrorString(e));
    }
    const int num_cu = slide_num_cu();
    if (!num_cu) WV_FAIL(WV_EHIP, "%s: device query failed", what);
    const int by_lds = std::max<int>(1, (int)((size_t)kMaxLdsBytes / (lds + 512)));
    const int per_cu = std::min(by_lds, std::max(1, minw * 256 / (2 * NT)));
    const int64_t planes = (int64_t)g.B * g.C;
    int64_t grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    g.coal = std::is_same<InT, uint8_t>::value && LAYOUT == 0 && R == 16 && g.W % 16 == 0 && g.nrun <= 16 &&
             (int64_t)g.H * g.W % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    g.nxcd = kXcds;
    if (grid < planes) grid -= grid % g.nxcd;      // persistent launch: same number of workgroups on every XCD
    if (grid <= 0 || grid % g.nxcd) g.nxcd = 1, grid = std::min<int64_t>(planes, (int64_t)num_cu * per_cu);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(2 * NT), lds, st, (const InT *)in, out, g, taps);
    WV_CHECK_LAUNCH(name);
    return WV_OK;
}

// The (input dtype, input layout, bf16 output) instantiation a call needs: go(InT{}, integral_constant<int, LAYOUT>{},
// bool_constant<BF16>{}).  NHWC means C == 3 here (slide_fits).
template <typename InT, typename Go>
static int slide_io_layout(const SwtShape &s, Go &go)
{
    using L0 = std::integral_constant<int, 0>;
    using L1 = std::integral_constant<int, 1>;
    const bool bf16 = s.out_dtype == WV_DT_BF16;
    if (s.in_layout == WV_LAYOUT_NHWC) return bf16 ? go(InT{}, L1{}, std::true_type{}) : go(InT{}, L1{}, std::false_type{});
    return bf16 ? go(InT{}, L0{}, std::true_type{}) : go(InT{}, L0{}, std::false_type{});
}
template <typename Go>
static int slide_io_dispatch(const SwtShape &s, Go go)
{
    return s.in_dtype == WV_DT_U8 ? slide_io_layout<uint8_t>(s, go) : slide_io_layout<float>(s, go);
}

}  // namespace wv
