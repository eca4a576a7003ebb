// Opt-in bf16 matrix-core path of the band-attention pooling head (eval mode) for gfx950.
//
// Same forward as head.hip (CrossAttentionBottleneckHead*.forward), with the numerical contract of a mixed-precision
// run: BOTH operands of every dense weight product -- K | V in-projection, attention out-projection, mlp.0, mlp.2,
// read-out -- are bf16 (round to nearest even), every product accumulates in fp32 on v_mfma_f32_32x32x16_bf16, and
// biases, residual adds, the softmax over the band tokens, both LayerNorms and GELU stay fp32.  Output fp32 [B][E].
//
// Structure: one launch per stage, as the general fp32 path.  With bf16 operands the products are 16x cheaper on the
// matrix pipes, so a fused front that streams all 10 E^2 weights per 32 rows (head_front.hip's design point) would be
// bound by that stream; here every weight tile is shared by 64 or 128 rows through LDS and the intermediates travel
// through HBM -- the widest one (the MLP hidden layer, used only as an operand) as bf16, which is the same numbers
// as rounding it when it is read.  The attention core, LayerNorm and mean-pool kernels are head.hip's (fp32 in/out).
// Weights are converted once (wv_band_attn_bf16_prepare), activations where they are staged as an operand; band
// features are taken as fp32 or bf16 and never copied.
#include "head.hpp"

namespace wv {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// eight consecutive operand elements on their way global -> registers -> LDS: fp32 sources are rounded when they are
// written to LDS, bf16 sources pass through
template <typename T> struct Raw8;
template <> struct Raw8<float> {
    f32x4 lo, hi;
    __device__ __forceinline__ void load(const float *p)
    {
        lo = *reinterpret_cast<const f32x4 *>(p);
        hi = *reinterpret_cast<const f32x4 *>(p + 4);
    }
    __device__ __forceinline__ bf16x8 packed() const
    {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (__bf16)lo[j];
            v[4 + j] = (__bf16)hi[j];
        }
        return v;
    }
};
template <> struct Raw8<__bf16> {
    bf16x8 v;
    __device__ __forceinline__ void load(const __bf16 *p) { v = *reinterpret_cast<const bf16x8 *>(p); }
    __device__ __forceinline__ bf16x8 packed() const { return v; }
};

// C[M][N] = epi(A[M][K] . W[N][K]^T + bias[N]), A fp32 or bf16, W bf16, C fp32 or bf16; epilogues: head.hpp (store_block, GELU through gelu_erf()).
// Block tile BM x BN (64 x 64 or 128 x 128), 4 waves as 2 x 2, wave tile in 32 x 32 blocks of v_mfma_f32_32x32x16_bf16:
// lane (r, h) feeds row r with k in [16 s + 8 h, 16 s + 8 h + 8) of MFMA s of a BK-wide K step (BK = 32 or 64) -- one
// 16-byte LDS read per fragment.  Two LDS stages; rows are padded by 8 bf16 (pitch 80 or 144 bytes): 16 lanes = 16 rows
// then start in 16 distinct 4-bank groups.  kchunk % BK == 0 (host); rows past M / N are clamped on load and skipped on
// store.  Split K (gridDim.z > 1, EPI_NONE and fp32 C only): slice z covers k in [z*kchunk, (z+1)*kchunk) and writes its
// partial product to C + z*M*N (bias in slice 0); the consumer (k_layernorm) adds the slices in index order.
template <int BM, int BN, int BK, int EPI, typename TA, typename TC>
__global__ __launch_bounds__(256) void k_gemm_bf16(const TA *__restrict__ A, const __bf16 *__restrict__ W,
                                                   const float *__restrict__ bias, const float *__restrict__ R, int rmod,
                                                   TC *__restrict__ C, int M, int N, int K, int kchunk)
{
    constexpr int LDP = BK + 8;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int CPR = BK / 8;                                          // 8-element chunks per row
    constexpr int CA = BM * CPR / 256, CB = BN * CPR / 256;              // chunks per thread per stage
    constexpr int STAGE = (BM + BN) * LDP;                               // [A tile | W tile]
    extern __shared__ float4 bsm4[];
    __bf16 *sm = reinterpret_cast<__bf16 *>(bsm4);
    {
        const int z = blockIdx.z;
        A += (size_t)z * kchunk;
        W += (size_t)z * kchunk;
        C += (size_t)z * M * N;
        if (z) bias = nullptr;
    }
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int r = lane & 31, h = lane >> 5;
    // XCD k gets the k-th contiguous eighth of the tile list (see k_gemm_panel): tiles that share A rows or W rows meet in one L2
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int total = gridDim.x * gridDim.y;
        if (total % 8 == 0) {
            const int lin = blockIdx.y * gridDim.x + blockIdx.x;
            const int tile = (lin % 8) * (total / 8) + lin / 8;
            by = tile / gridDim.x;
            bx = tile - by * gridDim.x;
        }
    }
    const int64_t m0 = (int64_t)by * BM, n0 = (int64_t)bx * BN;
    const int wm = (wv >> 1) * (BM / 2), wn = (wv & 1) * (BN / 2);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    // Operand tiles travel global -> registers -> LDS.  A K step's MFMAs are far shorter than a trip to memory, so the
    // registers are a ring of D tile sets: tile t + D is requested when tile t starts to be multiplied, and a set is
    // written to the free LDS stage one step before its tile is used.  Every request is issued unconditionally (past the
    // end the last tile is requested again) so that the counted waits the compiler places keep D - 1 sets in flight.
    constexpr int D = 3;
    Raw8<TA> ra[D][CA];
    Raw8<__bf16> rb[D][CB];
    const TA *ga[CA];
    const __bf16 *gb[CB];
    int so_a[CA], so_b[CB];
#pragma unroll
    for (int i = 0; i < CA; ++i) {
        const int ch = i * 256 + tid, row = ch / CPR, c8 = ch % CPR;
        ga[i] = A + min(m0 + row, (int64_t)M - 1) * K + 8 * c8;
        so_a[i] = row * LDP + 8 * c8;
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
        const int ch = i * 256 + tid, row = ch / CPR, c8 = ch % CPR;
        gb[i] = W + min(n0 + row, (int64_t)N - 1) * K + 8 * c8;
        so_b[i] = BM * LDP + row * LDP + 8 * c8;
    }
    const int nk = kchunk / BK;
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int k0 = min(u, nk - 1) * BK;
#pragma unroll
        for (int i = 0; i < CA; ++i) ra[u][i].load(ga[i] + k0);
#pragma unroll
        for (int i = 0; i < CB; ++i) rb[u][i].load(gb[i] + k0);
    }
#pragma unroll
    for (int i = 0; i < CA; ++i) *reinterpret_cast<bf16x8 *>(sm + so_a[i]) = ra[0][i].packed();
#pragma unroll
    for (int i = 0; i < CB; ++i) *reinterpret_cast<bf16x8 *>(sm + so_b[i]) = rb[0][i].packed();
    __syncthreads();
    for (int kt0 = 0; kt0 < nk; kt0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {   // u = kt % D: register set indices are compile-time constants
            const int kt = kt0 + u;
            if (kt < nk) {              // uniform
                const __bf16 *cur = sm + (kt & 1) * STAGE;
                __bf16 *nxt = sm + ((kt & 1) ^ 1) * STAGE;
                {   // set u went to LDS in the previous step: tile kt + D
                    const int k0 = min(kt + D, nk - 1) * BK;
#pragma unroll
                    for (int i = 0; i < CA; ++i) ra[u][i].load(ga[i] + k0);
#pragma unroll
                    for (int i = 0; i < CB; ++i) rb[u][i].load(gb[i] + k0);
                }
                const __bf16 *as = cur + (wm + r) * LDP + 8 * h;
                const __bf16 *bs = cur + BM * LDP + (wn + r) * LDP + 8 * h;
#pragma unroll
                for (int s = 0; s < BK / 16; ++s) {
                    bf16x8 av[TM], bv[TN];
#pragma unroll
                    for (int a = 0; a < TM; ++a) av[a] = *reinterpret_cast<const bf16x8 *>(as + a * 32 * LDP + 16 * s);
#pragma unroll
                    for (int b = 0; b < TN; ++b) bv[b] = *reinterpret_cast<const bf16x8 *>(bs + b * 32 * LDP + 16 * s);
#pragma unroll
                    for (int a = 0; a < TM; ++a)
#pragma unroll
                        for (int b = 0; b < TN; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[a], bv[b], acc[a][b], 0, 0, 0);
                }
                if (kt + 1 < nk) {   // tile kt + 1; the other stage was last read before the previous barrier
                    const int v = (u + 1) % D;   // constant once the loop over u is unrolled
#pragma unroll
                    for (int i = 0; i < CA; ++i) *reinterpret_cast<bf16x8 *>(nxt + so_a[i]) = ra[v][i].packed();
#pragma unroll
                    for (int i = 0; i < CB; ++i) *reinterpret_cast<bf16x8 *>(nxt + so_b[i]) = rb[v][i].packed();
                }
                __syncthreads();
            }
        }
    }
    const int64_t row0 = m0 + wm + 4 * h, col0 = n0 + wn + r;
    if (m0 + BM <= M && n0 + BN <= N) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) store_block<EPI, false, false>(acc[a][b], row0 + a * 32, col0 + b * 32, bias, R, rmod, C, M, N);
    } else {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) store_block<EPI, true, false>(acc[a][b], row0 + a * 32, col0 + b * 32, bias, R, rmod, C, M, N);
    }
}

// the bf16 copy of a weight matrix (round to nearest even), made once per parameter update
__global__ __launch_bounds__(256) void k_to_bf16(const float *__restrict__ src, __bf16 *__restrict__ dst, int64_t n8)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        Raw8<float> v;
        v.load(src + 8 * i);
        *reinterpret_cast<bf16x8 *>(dst + 8 * i) = v.packed();
    }
}

template <int BM, int BN, int BK, int EPI, typename TA, typename TC>
static void launch_tile(const TA *A, const __bf16 *W, const float *bias, const float *R, int rmod, TC *C, int M, int N, int K,
                        int ksplit, hipStream_t st)
{
    constexpr size_t lds = (size_t)2 * (BM + BN) * (BK + 8) * 2;
    auto kern = k_gemm_bf16<BM, BN, BK, EPI, TA, TC>;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((unsigned)ceil_div(N, BN), (unsigned)ceil_div(M, BM), (unsigned)ksplit);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, A, W, bias, R, rmod, C, M, N, K, K / ksplit);
}

// the bf16 precision of head_run_stages: the tile head_plan chose for the product, nothing decided here.
// ksplit > 1: C receives that many [M][N] partial products (see k_gemm_bf16); K / ksplit is then a multiple of 64
struct PathBf16 {
    using Hidden = __bf16;
    template <int EPI, typename TA, typename TC>
    static void gemm(GemmPlan g, const TA *A, const __bf16 *W, const float *bias, const float *R, int rmod, TC *C, int M, int N,
                     int K, hipStream_t st)
    {
        switch (g.kernel) {
        case Gemm::bf128k32: return launch_tile<128, 128, 32, EPI>(A, W, bias, R, rmod, C, M, N, K, g.ksplit, st);
        case Gemm::bf64k64: return launch_tile<64, 64, 64, EPI>(A, W, bias, R, rmod, C, M, N, K, g.ksplit, st);
        case Gemm::bf64k32: return launch_tile<64, 64, 32, EPI>(A, W, bias, R, rmod, C, M, N, K, g.ksplit, st);
        default: return;   // an fp32 kernel: head_plan(HeadPrec::bf16) never answers one
        }
    }
};

// prepared blob: [Qp fp32 Nq*E | in_proj rows E..3E | attn_out | mlp.0 | mlp.2 | out_proj], weights bf16, 256-byte aligned
struct Bf16Blob {
    float *Qp;
    __bf16 *wkv, *wo, *w0, *w2, *wout;
    size_t bytes;
};

static Bf16Blob carve_blob(const wv_head_params *p, void *base)
{
    const size_t E = p->embed_dim, Nq = p->num_queries;
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        void *r = base ? (char *)base + off : nullptr;
        off += align_up((int64_t)nbytes, 256);
        return r;
    };
    Bf16Blob b;
    b.Qp = (float *)take(Nq * E * sizeof(float));
    b.wkv = (__bf16 *)take(2 * E * E * 2);
    b.wo = (__bf16 *)take(E * E * 2);
    b.w0 = (__bf16 *)take(4 * E * E * 2);
    b.w2 = (__bf16 *)take(4 * E * E * 2);
    b.wout = (__bf16 *)take(E * (p->pool_mean ? E : Nq * E) * 2);
    b.bytes = off;
    return b;
}

}  // namespace wv

using namespace wv;

extern "C" size_t wv_band_attn_bf16_prepared_bytes(const wv_head_params *p)
{
    if (!p) return 0;
    const HeadPlan pl = head_plan(p, 1, HeadPrec::bf16);
    if (pl.rc) {
        set_error("%s", pl.why);
        return 0;
    }
    return carve_blob(p, nullptr).bytes;
}

extern "C" int wv_band_attn_bf16_prepare(const wv_head_params *p, void *prepared_out, void *stream)
{
    const HeadPlan pl = head_plan(p, 1, HeadPrec::bf16);
    if (pl.rc) WV_FAIL(pl.rc, "%s", pl.why);
    WV_REQUIRE(prepared_out, "band_attn_bf16_prepare: null buffer");
    hipStream_t st = (hipStream_t)stream;
    const size_t E = p->embed_dim, Nq = p->num_queries;
    const Bf16Blob b = carve_blob(p, prepared_out);
    launch_qproj(p, b.Qp, st);
    const struct { const float *src; __bf16 *dst; size_t n; } mats[] = {
        {p->in_proj_w + E * E, b.wkv, 2 * E * E}, {p->attn_out_w, b.wo, E * E},           {p->mlp0_w, b.w0, 4 * E * E},
        {p->mlp2_w, b.w2, 4 * E * E},             {p->out_w, b.wout, E * (p->pool_mean ? E : Nq * E)},
    };
    for (const auto &m : mats) {   // every size is a multiple of E, hence of 8
        const int64_t n8 = (int64_t)(m.n / 8);
        hipLaunchKernelGGL(k_to_bf16, dim3((unsigned)std::min<int64_t>(ceil_div(n8, 256), 1024)), dim3(256), 0, st, m.src, m.dst, n8);
    }
    WV_CHECK_LAUNCH("band_attn_bf16_prepare");
    return WV_OK;
}

extern "C" size_t wv_band_attn_pool_bf16_workspace_bytes(const wv_head_params *p, int B)
{
    return head_plan(p, B, HeadPrec::bf16).ws.bytes;
}

extern "C" int wv_band_attn_pool_bf16(const wv_head_params *p, const void *prepared_bf16, const void *feats, int feat_dtype,
                                      int B, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    const HeadPlan pl = head_plan(p, B, HeadPrec::bf16);
    if (pl.rc) WV_FAIL(pl.rc, "%s", pl.why);
    WV_REQUIRE(prepared_bf16, "band_attn_pool_bf16: null prepared blob (wv_band_attn_bf16_prepare makes it)");
    WV_REQUIRE(feat_dtype == WV_DT_F32 || feat_dtype == WV_DT_BF16,
               "band_attn_pool_bf16: feat_dtype=%d (WV_DT_F32 or WV_DT_BF16)", feat_dtype);
    WV_REQUIRE(feats && out, "band_attn_pool_bf16: null buffer");
    WV_REQUIRE((int64_t)B * std::max(p->num_queries, p->num_tokens) < (1ll << 31), "band_attn_pool_bf16: B=%d too large", B);
    if (B == 0) return WV_OK;
    if (!workspace || workspace_bytes < pl.ws.bytes)
        WV_FAIL(WV_ENOMEM, "band_attn_pool_bf16: workspace %zu < %zu bytes", workspace_bytes, pl.ws.bytes);
    const Bf16Blob b = carve_blob(p, const_cast<void *>(prepared_bf16));
    const HeadWeights<__bf16> w{b.wkv, b.wo, b.w0, b.w2, b.wout};
    hipStream_t st = (hipStream_t)stream;
    if (feat_dtype == WV_DT_BF16)
        head_run_stages<PathBf16>(p, pl, w, b.Qp, reinterpret_cast<const __bf16 *>(feats), B, out, workspace, st);
    else head_run_stages<PathBf16>(p, pl, w, b.Qp, reinterpret_cast<const float *>(feats), B, out, workspace, st);
    WV_CHECK_LAUNCH("band_attn_pool_bf16");
    return WV_OK;
}
