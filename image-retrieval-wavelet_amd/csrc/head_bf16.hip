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
#include "common.hpp"

namespace wv {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

enum { EPI_NONE = 0, EPI_GELU = 1, EPI_ADD_ROW = 2, EPI_ADD_BCAST = 3 };

// head.hip: the stages both precisions share
int head_check_params(const wv_head_params *p, int B);
void head_launch_qproj(const wv_head_params *p, float *Qp, hipStream_t st);
size_t head_attn_core_lds(const wv_head_params *p);
void head_launch_attn_core(const wv_head_params *p, const float *Qp, const float *KV, float *ctx, int B, hipStream_t st);
void head_launch_mean_rows(const float *x, float *y, int64_t groups, int n, int E, hipStream_t st);
void launch_layernorm(const float *x, const float *w, const float *b, float *y, int64_t rows, int E, float eps, int nparts,
                      hipStream_t st);

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

// Epilogue of one 32 x 32 accumulator block: element e of this lane is row row0 + (e & 3) + 8 (e >> 2), column col.
// GUARD = false (interior tiles): no bounds checks, so the 16 residual loads are in flight together; the guarded form
// waits for each load before it issues the next.
template <int EPI, bool GUARD, typename TC>
__device__ __forceinline__ void store_block(const f32x16 &acc, int64_t row0, int64_t col, const float *__restrict__ bias,
                                            const float *__restrict__ R, int rmod, TC *__restrict__ C, int M, int N)
{
    if (GUARD && col >= N) return;
    const float bsv = bias ? bias[col] : 0.f;
    float res[16];
    if (EPI == EPI_ADD_BCAST) {
        // R row = output row mod rmod, carried along the lane's rows (steps of 1, 1, 1, 5) instead of 16 divisions
        const uint32_t m = (uint32_t)rmod, d1 = 1u % m, d5 = 5u % m;   // rows < 2^31 (host check)
        uint32_t q = (uint32_t)row0 % m;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            res[e] = GUARD && row0 + (e & 3) + 8 * (e >> 2) >= M ? 0.f : R[(int64_t)q * N + col];
            q += (e & 3) == 3 ? d5 : d1;
            q -= q >= m ? m : 0u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
            res[e] = EPI == EPI_ADD_ROW && !(GUARD && row >= M) ? R[row * N + col] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
        float v = acc[e] + bsv;
        if (EPI == EPI_GELU) v = gelu_erf(v);
        if (EPI == EPI_ADD_ROW || EPI == EPI_ADD_BCAST) v += res[e];
        if (!GUARD || row < M) C[row * N + col] = (TC)v;
    }
}

// C[M][N] = epi(A[M][K] . W[N][K]^T + bias[N]), A fp32 or bf16, W bf16, C fp32 or bf16; epilogues as k_gemm_nt.
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
            for (int b = 0; b < TN; ++b) store_block<EPI, false>(acc[a][b], row0 + a * 32, col0 + b * 32, bias, R, rmod, C, M, N);
    } else {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) store_block<EPI, true>(acc[a][b], row0 + a * 32, col0 + b * 32, bias, R, rmod, C, M, N);
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

// ksplit > 1: C receives that many [M][N] partial products (see k_gemm_bf16); K / ksplit must be a multiple of 64
template <int EPI, typename TA, typename TC>
static void launch_gemm_bf16(const TA *A, const __bf16 *W, const float *bias, const float *R, int rmod, TC *C, int M, int N,
                             int K, hipStream_t st, int ksplit = 1)
{
    // 128 x 128 tiles when they still give every CU one; the 64-wide K step whenever K allows it.  WV_HEAD_BF16=tile64 /
    // tile128 and WV_HEAD_BF16_BK=32 pin a variant (tests, A/B runs)
    const char *pin = ::wv::tune("WV_HEAD_BF16"), *pin_bk = ::wv::tune("WV_HEAD_BF16_BK");
    bool big = ceil_div(M, 128) * ceil_div(N, 128) >= 256;
    if (pin && !strcmp(pin, "tile64")) big = false;
    if (pin && !strcmp(pin, "tile128")) big = true;
    const bool bk64 = (K / ksplit) % 64 == 0 && !(pin_bk && !strcmp(pin_bk, "32"));
    if (big) launch_tile<128, 128, 32, EPI>(A, W, bias, R, rmod, C, M, N, K, ksplit, st);   // the 64-wide step costs it a workgroup per CU
    else if (bk64) launch_tile<64, 64, 64, EPI>(A, W, bias, R, rmod, C, M, N, K, ksplit, st);
    else launch_tile<64, 64, 32, EPI>(A, W, bias, R, rmod, C, M, N, K, ksplit, st);
}

// Slices the read-out product is cut into (1 = no split): M = B rows give few tiles, so K is cut until about every CU has
// a few workgroups.  C must then hold that many [M][N] partials.
static int readout_ksplit_bf16(int M, int N, int K)
{
    if (ceil_div(M, 128) * ceil_div(N, 128) >= 256) return 1;
    const int64_t tiles = ceil_div(M, 64) * ceil_div(N, 64);
    for (int ks = 8; ks >= 2; ks >>= 1)
        if (K % (ks * 64) == 0 && K / ks >= 128 && tiles * ks <= 1024) return ks;
    return 1;
}

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

struct Bf16Ws {
    float *KV, *ctx, *x1, *x1n, *x2, *pooled, *pre;
    __bf16 *hid;
    size_t bytes;
};

static Bf16Ws carve_ws(const wv_head_params *p, int B, void *base)
{
    const size_t E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    const size_t rows = (size_t)B * Nq;
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        void *r = base ? (char *)base + off : nullptr;
        off += align_up((int64_t)nbytes, 256);
        return r;
    };
    Bf16Ws w;
    w.KV = (float *)take(S * B * 2 * E * sizeof(float));
    w.ctx = (float *)take(rows * E * sizeof(float));
    w.x1 = (float *)take(rows * E * sizeof(float));
    w.x1n = (float *)take(rows * E * sizeof(float));
    w.hid = (__bf16 *)take(rows * 4 * E * 2);
    w.x2 = (float *)take(rows * E * sizeof(float));
    w.pooled = (float *)take((size_t)B * E * sizeof(float));
    w.pre = (float *)take((size_t)B * E * 8 * sizeof(float));   // up to 8 split-K partials of the read-out product
    w.bytes = off;
    return w;
}

}  // namespace wv

using namespace wv;

static int check_head_bf16(const wv_head_params *p, int B)
{
    int rc = head_check_params(p, B);
    if (rc) return rc;
    WV_REQUIRE(p->embed_dim % 32 == 0, "band_attn_pool_bf16: embed_dim=%d must be a multiple of 32", p->embed_dim);
    if (head_attn_core_lds(p) > (size_t)kMaxLdsBytes)
        WV_FAIL(WV_ENOTSUP, "band_attn_pool_bf16: %d tokens x %d queries at embed_dim=%d do not fit the attention kernel's LDS",
                p->num_tokens, p->num_queries, p->embed_dim);
    return WV_OK;
}

extern "C" size_t wv_band_attn_bf16_prepared_bytes(const wv_head_params *p)
{
    if (!p || check_head_bf16(p, 1)) return 0;
    return carve_blob(p, nullptr).bytes;
}

extern "C" int wv_band_attn_bf16_prepare(const wv_head_params *p, void *prepared_out, void *stream)
{
    int rc = check_head_bf16(p, 1);
    if (rc) return rc;
    WV_REQUIRE(prepared_out, "band_attn_bf16_prepare: null buffer");
    hipStream_t st = (hipStream_t)stream;
    const size_t E = p->embed_dim, Nq = p->num_queries;
    const Bf16Blob b = carve_blob(p, prepared_out);
    head_launch_qproj(p, b.Qp, st);
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
    if (!p || B <= 0) return 0;
    return carve_ws(p, B, nullptr).bytes;
}

template <typename TF>
static void run_head_bf16(const wv_head_params *p, const Bf16Blob &w, const TF *feats, int B, float *out, const Bf16Ws &ws,
                          hipStream_t st)
{
    const int E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens, rows = B * Nq;
    // K | V projection of all S*B tokens
    launch_gemm_bf16<EPI_NONE>(feats, w.wkv, p->in_proj_b + E, (const float *)nullptr, 1, ws.KV, S * B, 2 * E, E, st);
    head_launch_attn_core(p, w.Qp, ws.KV, ws.ctx, B, st);
    // x1 = q_eff + ctx @ Wo^T + bo ; x1n = LN1(x1)
    launch_gemm_bf16<EPI_ADD_BCAST>(ws.ctx, w.wo, p->attn_out_b, p->q_eff, Nq, ws.x1, rows, E, E, st);
    launch_layernorm(ws.x1, p->norm1_w, p->norm1_b, ws.x1n, (int64_t)rows, E, p->ln_eps, 1, st);
    // x2 = x1n + GELU(x1n @ W0^T + b0) @ W2^T + b2; the hidden layer is an operand only: kept as bf16
    launch_gemm_bf16<EPI_GELU>(ws.x1n, w.w0, p->mlp0_b, (const float *)nullptr, 1, ws.hid, rows, 4 * E, E, st);
    launch_gemm_bf16<EPI_ADD_ROW>(ws.hid, w.w2, p->mlp2_b, ws.x1n, 1, ws.x2, rows, E, 4 * E, st);
    // read-out: concat (a [B][Nq*E] view of x2) or mean over the queries, then Linear + LN2
    const float *ro_in = ws.x2;
    int ro_k = Nq * E;
    if (p->pool_mean) {
        head_launch_mean_rows(ws.x2, ws.pooled, (int64_t)B, Nq, E, st);
        ro_in = ws.pooled;
        ro_k = E;
    }
    const int ks = readout_ksplit_bf16(B, E, ro_k);
    launch_gemm_bf16<EPI_NONE>(ro_in, w.wout, p->out_b, (const float *)nullptr, 1, ws.pre, B, E, ro_k, st, ks);
    launch_layernorm(ws.pre, p->norm2_w, p->norm2_b, out, (int64_t)B, E, p->ln_eps, ks, st);
}

extern "C" int wv_band_attn_pool_bf16(const wv_head_params *p, const void *prepared_bf16, const void *feats, int feat_dtype,
                                      int B, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_head_bf16(p, B);
    if (rc) return rc;
    WV_REQUIRE(prepared_bf16, "band_attn_pool_bf16: null prepared blob (wv_band_attn_bf16_prepare makes it)");
    WV_REQUIRE(feat_dtype == WV_DT_F32 || feat_dtype == WV_DT_BF16,
               "band_attn_pool_bf16: feat_dtype=%d (WV_DT_F32 or WV_DT_BF16)", feat_dtype);
    WV_REQUIRE(feats && out, "band_attn_pool_bf16: null buffer");
    WV_REQUIRE((int64_t)B * std::max(p->num_queries, p->num_tokens) < (1ll << 31), "band_attn_pool_bf16: B=%d too large", B);
    if (B == 0) return WV_OK;
    const size_t need = carve_ws(p, B, nullptr).bytes;
    if (!workspace || workspace_bytes < need)
        WV_FAIL(WV_ENOMEM, "band_attn_pool_bf16: workspace %zu < %zu bytes", workspace_bytes, need);
    const Bf16Blob w = carve_blob(p, const_cast<void *>(prepared_bf16));
    const Bf16Ws ws = carve_ws(p, B, workspace);
    if (feat_dtype == WV_DT_BF16) run_head_bf16(p, w, reinterpret_cast<const __bf16 *>(feats), B, out, ws, (hipStream_t)stream);
    else run_head_bf16(p, w, reinterpret_cast<const float *>(feats), B, out, ws, (hipStream_t)stream);
    WV_CHECK_LAUNCH("band_attn_pool_bf16");
    return WV_OK;
}
