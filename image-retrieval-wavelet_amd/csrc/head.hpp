// Band-attention head, host side and shared device code: what runs for (parameters, batch, precision) -- the planner --,
// where each intermediate lies in the caller's workspace, the one GEMM epilogue, the one stage sequence, and the interface
// between head.hip (fp32 products, the stages every precision shares, entry points), head_front.hip (the one-launch
// front) and head_bf16.hip (bf16 products).  Every dispatch rule lives in head_plan(): the entry points ask it and the
// launchers run what it answers.
#pragma once
#include "common.hpp"
#include "head_args.hpp"

namespace wv {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;   // native vector: arrays of it stay in registers

// C[M][N] = epi(A[M][K] . W[N][K]^T + bias[N])
//   EPI_ADD_ROW   : + R[m][n]                    (residual of the same shape)
//   EPI_ADD_BCAST : + R[(m % rmod)][n]           (query tokens broadcast over the batch)
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_ADD_ROW = 2, EPI_ADD_BCAST = 3 };

// Epilogue of one 32 x 32 accumulator block: element e of this lane is row row0 + (e & 3) + 8 (e >> 2), column col.
// GUARD = false (interior tiles): no bounds checks, so the 16 residual loads are in flight together; the guarded form
// waits for each load before it issues the next.  ERFF: GELU through the library erff (the fp32 separate launches) or
// through gelu_erf() (common.hpp: the bf16 products).
template <int EPI, bool GUARD, bool ERFF, typename TC>
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
        if (EPI == EPI_GELU) v = ERFF ? 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)) : gelu_erf(v);
        if (EPI == EPI_ADD_ROW || EPI == EPI_ADD_BCAST) v += res[e];
        if (!GUARD || row < M) C[row * N + col] = (TC)v;
    }
}

// ---- the plan
enum class HeadPrec { f32, bf16 };

// the exact kernel of one product; the fp32 names are the values WV_GEMM takes (diagnostic library: tests, tuning)
enum class Gemm {
    none,
    nt64, nt128,                // k_gemm_nt<1,1> / <2,2>: no LDS, K % 8 == 0
    lds64, lds128x64, lds128,   // k_gemm_lds<64,64> / <128,64> / <128,128>: K % 32 == 0, M >= 64
    panel32, panel64,           // k_gemm_panel<32> / <64>: K % 64 == 0, N % 96 == 0, M >= 128
    bf64k64, bf64k32, bf128k32, // k_gemm_bf16<64,64,64> / <64,64,32> / <128,128,32>
};
struct GemmPlan {
    Gemm kernel;
    int ksplit;                 // slices along K (1 = no split); C then holds that many [M][N] partials
};
enum { P_KV = 0, P_OUT, P_MLP0, P_MLP2, P_READOUT, P_COUNT };   // the five products

// byte offsets of the intermediates in the caller's workspace, every slot 256-byte aligned
struct HeadWs {
    size_t Qp, KV, ctx, x1, x1n, hid, x2, pooled, pre, bytes;
};
template <typename T> inline T *ws_at(void *base, size_t off) { return reinterpret_cast<T *>((char *)base + off); }

struct HeadPlan {
    int rc;                     // WV_OK, or the code of the refusal ...
    char why[256];              // ... and its text
    bool front;                 // everything before the read-out in one launch (head_front.hip)
    GemmPlan gemm[P_COUNT];
    size_t attn_lds;            // dynamic LDS of k_attn_core
    HeadWs ws;
};

// head_front.hip: the fused front (band features -> x2 in one launch) and its prepared weight stream
bool head_front_has_kernel(const wv_head_params *p);
size_t head_front_prepared_bytes(const wv_head_params *p);
int head_front_prepare(const wv_head_params *p, void *prepared, hipStream_t st);
void head_front_launch(const wv_head_params *p, const float *feats, int B, float *x2, hipStream_t st);

// head.hip: the stages both precisions share
void launch_qproj(const wv_head_params *p, float *Qp, hipStream_t st);
void launch_attn_core(const wv_head_params *p, const HeadPlan &pl, const float *Qp, const float *KV, float *ctx, int B, hipStream_t st);
void launch_layernorm(const float *x, const float *w, const float *b, float *y, int64_t rows, int E, float eps, int nparts,
                      hipStream_t st);
void launch_mean_rows(const float *x, float *y, int64_t groups, int n, int E, hipStream_t st);
// C[M][N] = A[M][K] . W[N][K]^T + bias[N] on the fp32 kernel g names (no epilogue): for head_attn.hip
void launch_gemm_f32(GemmPlan g, const float *A, const float *W, const float *bias, float *C, int M, int N, int K, hipStream_t st);

// The fp32 layout keeps a leading slot for the projected queries; the bf16 one has none (they come with its prepared
// blob) and holds the MLP hidden layer, an operand only, as bf16.
inline HeadWs head_ws_layout(const wv_head_params *p, int B, HeadPrec prec)
{
    const size_t E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    const size_t rows = (size_t)B * Nq;
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        const size_t at = off;
        off += align_up((int64_t)nbytes, 256);
        return at;
    };
    HeadWs w;
    w.Qp = take(prec == HeadPrec::f32 ? Nq * E * sizeof(float) : 0);
    w.KV = take(S * B * 2 * E * sizeof(float));
    w.ctx = take(rows * E * sizeof(float));
    w.x1 = take(rows * E * sizeof(float));
    w.x1n = take(rows * E * sizeof(float));
    w.hid = take(rows * 4 * E * (prec == HeadPrec::f32 ? sizeof(float) : 2));
    w.x2 = take(rows * E * sizeof(float));
    w.pooled = take((size_t)B * E * sizeof(float));
    w.pre = take((size_t)B * E * 8 * sizeof(float));   // up to 8 split-K partials of the read-out product
    w.bytes = off;
    return w;
}

// wv_band_attn_maps keeps three of them: Qp | K (| V) | ctx, sized for the call that asks for every output
struct HeadMapsWs {
    size_t Qp, KV, ctx, bytes;
};
inline HeadMapsWs head_maps_ws_layout(const wv_head_params *p, int B)
{
    const size_t E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    HeadMapsWs w;
    w.Qp = 0;
    w.KV = w.Qp + align_up((int64_t)(Nq * E * sizeof(float)), 256);
    w.ctx = w.KV + align_up((int64_t)(S * B * 2 * E * sizeof(float)), 256);
    w.bytes = w.ctx + align_up((int64_t)((size_t)B * Nq * E * sizeof(float)), 256);
    return w;
}

inline bool gemm_fits(Gemm g, int64_t M, int N, int K)
{
    if (g == Gemm::panel32 || g == Gemm::panel64) return K % 64 == 0 && N % 96 == 0 && M >= 128;
    if (g == Gemm::lds64 || g == Gemm::lds128x64 || g == Gemm::lds128) return K % 32 == 0 && M >= 64;
    return g == Gemm::nt64 || g == Gemm::nt128;
}

// fp32 product: the pinned kernel where the product meets its requirements, else by the measured rules
inline Gemm gemm_f32(int64_t M, int N, int K, const char *pin)
{
    static const struct { const char *name; Gemm g; } names[] = {
        {"nt64", Gemm::nt64},       {"nt128", Gemm::nt128},     {"lds64", Gemm::lds64},    {"lds128x64", Gemm::lds128x64},
        {"lds128", Gemm::lds128},   {"panel32", Gemm::panel32}, {"panel64", Gemm::panel64},
    };
    for (const auto &n : names)
        if (pin && !strcmp(pin, n.name) && gemm_fits(n.g, M, N, K)) return n.g;
    const int64_t panels = ceil_div(M, 128) * ceil_div(N, 96);
    if (gemm_fits(Gemm::panel64, M, N, K) && panels >= 256) {
        // one workgroup per CU: nothing else hides the stage hand-over, so take the long K step
        return panels < 512 ? Gemm::panel64 : Gemm::panel32;
    }
    // measured on MI355X at the head's shapes: short-K, wide-N products (mlp.0: K=384, N=1536) run faster on
    // the LDS-free kernel (118 vs 142 us); everything else on the LDS-tiled one
    const bool prefer_stream = K <= 512 && N >= 1024;
    if (gemm_fits(Gemm::lds64, M, N, K) && !prefer_stream) {
        // largest tile that still gives every CU about two workgroups
        if (ceil_div(M, 128) * ceil_div(N, 128) >= 512) return Gemm::lds128;
        if (ceil_div(M, 128) * ceil_div(N, 64) >= 384) return Gemm::lds128x64;
        return Gemm::lds64;
    }
    // big tile when it still yields >= 256 workgroups, else the small one
    return ceil_div(M, 128) * ceil_div(N, 128) >= 256 ? Gemm::nt128 : Gemm::nt64;
}

// Slices the fp32 read-out product is cut into (1 = no split): short-M products leave most CUs without a
// panel, so K is cut until about every CU has one.  Any WV_GEMM pin disables the split.
inline int readout_ksplit_f32(int64_t M, int N, int K, const char *pin)
{
    if (pin || K % 64 || N % 96 || M < 128) return 1;
    const int64_t panels = ceil_div(M, 128) * ceil_div(N, 96);
    for (int ks = 8; ks >= 2; ks >>= 1)
        if (K % (ks * 64) == 0 && K / ks >= 128 && panels * ks <= 384) return ks;
    return 1;
}

// bf16 product: 128 x 128 tiles when they still give every CU one; the 64-wide K step whenever K (per slice) allows it.
// WV_HEAD_BF16=tile64 / tile128 and WV_HEAD_BF16_BK=32 pin a variant (tests, A/B runs)
inline Gemm gemm_bf16(int64_t M, int N, int K, int ksplit, const char *pin, const char *pin_bk)
{
    bool big = ceil_div(M, 128) * ceil_div(N, 128) >= 256;
    if (pin && !strcmp(pin, "tile64")) big = false;
    if (pin && !strcmp(pin, "tile128")) big = true;
    const bool bk64 = (K / ksplit) % 64 == 0 && !(pin_bk && !strcmp(pin_bk, "32"));
    if (big) return Gemm::bf128k32;   // the 64-wide step costs it a workgroup per CU
    return bk64 ? Gemm::bf64k64 : Gemm::bf64k32;
}

// Slices the bf16 read-out product is cut into (1 = no split): M = B rows give few tiles, so K is cut until about every
// CU has a few workgroups.
inline int readout_ksplit_bf16(int64_t M, int N, int K)
{
    if (ceil_div(M, 128) * ceil_div(N, 128) >= 256) return 1;
    const int64_t tiles = ceil_div(M, 64) * ceil_div(N, 64);
    for (int ks = 8; ks >= 2; ks >>= 1)
        if (K % (ks * 64) == 0 && K / ks >= 128 && tiles * ks <= 1024) return ks;
    return 1;
}

#define WV_PLAN_REFUSE(pl, code, ...) ((pl).rc = (code), snprintf((pl).why, sizeof((pl).why), __VA_ARGS__), false)

// the argument check of every head entry point: false with pl.rc / pl.why set when the parameters are refused
inline bool head_check_params(const wv_head_params *p, int B, HeadPlan &pl)
{
    if ((pl.rc = head_attn_args_refusal(p, B, "band_attn_pool", pl.why, sizeof(pl.why))) != WV_OK) return false;
    if (!(p->norm1_w && p->norm1_b && p->mlp0_w && p->mlp0_b && p->mlp2_w && p->mlp2_b && p->out_w && p->out_b && p->norm2_w &&
          p->norm2_b))
        return WV_PLAN_REFUSE(pl, WV_EINVAL, "band_attn_pool: null weight pointer");
    return true;
}

// THE rule: what wv_band_attn_pool (f32) / wv_band_attn_pool_bf16 run for parameters p and a batch of B samples, or why
// they refuse.  Every WV_HEAD_FRONT, WV_GEMM, WV_HEAD_BF16 and WV_HEAD_BF16_BK read (diagnostic library) happens here.
// The workspace layout is filled in for any non-null p and B > 0, refused or not (the *_workspace_bytes entry points).
inline HeadPlan head_plan(const wv_head_params *p, int B, HeadPrec prec)
{
    HeadPlan pl{};
    if (p && B > 0) pl.ws = head_ws_layout(p, B, prec);
    if (!head_check_params(p, B, pl)) return pl;
    const int E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    const char *what = prec == HeadPrec::bf16 ? "band_attn_pool_bf16" : "band_attn_pool";
    if (prec == HeadPrec::bf16 && E % 32) {
        WV_PLAN_REFUSE(pl, WV_EINVAL, "%s: embed_dim=%d must be a multiple of 32", what, E);
        return pl;
    }
    // k_attn_core keeps kv[S][2E + 4] | q[Nq][E] | P[Nq][heads][S] in LDS
    pl.attn_lds = head_attn_lds_bytes(p);
    if (pl.attn_lds > (size_t)kMaxLdsBytes) {
        WV_PLAN_REFUSE(pl, WV_ENOTSUP, "%s: %d tokens x %d queries at embed_dim=%d do not fit the attention kernel's LDS", what, S, Nq, E);
        return pl;
    }
    if (B <= 0) return pl;

    const int64_t rows = (int64_t)B * Nq;
    const int ro_k = p->pool_mean ? E : Nq * E;   // read-out: the mean over the queries, or a [B][Nq*E] view of x2
    if (prec == HeadPrec::bf16) {
        const char *pin = ::wv::tune("WV_HEAD_BF16"), *pin_bk = ::wv::tune("WV_HEAD_BF16_BK");
        const int ks = readout_ksplit_bf16(B, E, ro_k);
        pl.gemm[P_KV] = {gemm_bf16((int64_t)S * B, 2 * E, E, 1, pin, pin_bk), 1};
        pl.gemm[P_OUT] = {gemm_bf16(rows, E, E, 1, pin, pin_bk), 1};
        pl.gemm[P_MLP0] = {gemm_bf16(rows, 4 * E, E, 1, pin, pin_bk), 1};
        pl.gemm[P_MLP2] = {gemm_bf16(rows, E, 4 * E, 1, pin, pin_bk), 1};
        pl.gemm[P_READOUT] = {gemm_bf16(B, E, ro_k, ks, pin, pin_bk), ks};
        return pl;
    }
    // prepared weights: everything up to x2 in one launch when the batch fills the chip (WV_HEAD_FRONT=0 / 1 pins the
    // separate launches / the one-launch front for tests and A/B runs).  A workgroup of the front runs its 32 rows
    // through all 5,808 MFMAs of a wave whatever the batch: ~215 us even for one sample.  The separate launches spread a
    // small batch over the whole chip instead; measured crossover on MI355X (Nq = 4: B = 1024 -> 241 vs 217 us,
    // B = 1536 -> 252 vs 317 us): from about 9/16 of the 256 CUs on, the one-launch front wins.
    const char *front = ::wv::tune("WV_HEAD_FRONT");
    if (p->prepared && head_front_has_kernel(p) && !(front && !strcmp(front, "0")))
        pl.front = (front && !strcmp(front, "1")) || ceil_div(B, 32 / Nq) >= 144;
    const char *pin = ::wv::tune("WV_GEMM");
    const int ks = readout_ksplit_f32(B, E, ro_k, pin);
    pl.gemm[P_KV] = {gemm_f32((int64_t)S * B, 2 * E, E, pin), 1};
    pl.gemm[P_OUT] = {gemm_f32(rows, E, E, pin), 1};
    pl.gemm[P_MLP0] = {gemm_f32(rows, 4 * E, E, pin), 1};
    pl.gemm[P_MLP2] = {gemm_f32(rows, E, 4 * E, pin), 1};
    pl.gemm[P_READOUT] = {ks > 1 ? Gemm::panel64 : gemm_f32(B, E, ro_k, pin), ks};
    return pl;
}

// ---- the stage sequence, written once.  Path gives the precision: Path::gemm<EPI>(GemmPlan, A, W, bias, R, rmod, C, M, N,
// K, stream) launches one product, Path::Hidden is the element type of the MLP hidden layer (an operand only).
template <typename TW> struct HeadWeights {
    const TW *kv, *out, *mlp0, *mlp2, *readout;   // in_proj rows E..3E | attn out_proj | mlp.0 | mlp.2 | out_proj
};

template <typename Path, typename TF, typename TW>
inline void head_run_stages(const wv_head_params *p, const HeadPlan &pl, const HeadWeights<TW> &w, const float *Qp, const TF *feats,
                            int B, float *out, void *workspace, hipStream_t st)
{
    using TH = typename Path::Hidden;
    const int E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens, rows = B * Nq;
    const float *none = nullptr;
    float *KV = ws_at<float>(workspace, pl.ws.KV), *ctx = ws_at<float>(workspace, pl.ws.ctx), *x1 = ws_at<float>(workspace, pl.ws.x1);
    float *x1n = ws_at<float>(workspace, pl.ws.x1n), *x2 = ws_at<float>(workspace, pl.ws.x2), *pre = ws_at<float>(workspace, pl.ws.pre);
    TH *hid = ws_at<TH>(workspace, pl.ws.hid);
    if (pl.front) {
        head_front_launch(p, reinterpret_cast<const float *>(feats), B, x2, st);
    } else {
        // K | V projection of all S*B tokens: rows E..3E of in_proj_weight
        Path::template gemm<EPI_NONE>(pl.gemm[P_KV], feats, w.kv, p->in_proj_b + E, none, 1, KV, S * B, 2 * E, E, st);
        launch_attn_core(p, pl, Qp, KV, ctx, B, st);
        // x1 = q_eff + ctx @ Wo^T + bo ; x1n = LN1(x1)
        Path::template gemm<EPI_ADD_BCAST>(pl.gemm[P_OUT], ctx, w.out, p->attn_out_b, p->q_eff, Nq, x1, rows, E, E, st);
        launch_layernorm(x1, p->norm1_w, p->norm1_b, x1n, (int64_t)rows, E, p->ln_eps, 1, st);
        // x2 = x1n + GELU(x1n @ W0^T + b0) @ W2^T + b2
        Path::template gemm<EPI_GELU>(pl.gemm[P_MLP0], x1n, w.mlp0, p->mlp0_b, none, 1, hid, rows, 4 * E, E, st);
        Path::template gemm<EPI_ADD_ROW>(pl.gemm[P_MLP2], hid, w.mlp2, p->mlp2_b, x1n, 1, x2, rows, E, 4 * E, st);
    }
    // read-out: concat (a [B][Nq*E] view of x2) or mean over the queries, then Linear + LN2
    const float *ro_in = x2;
    if (p->pool_mean) {
        float *pooled = ws_at<float>(workspace, pl.ws.pooled);
        launch_mean_rows(x2, pooled, (int64_t)B, Nq, E, st);
        ro_in = pooled;
    }
    Path::template gemm<EPI_NONE>(pl.gemm[P_READOUT], ro_in, w.readout, p->out_b, none, 1, pre, B, E, p->pool_mean ? E : Nq * E, st);
    launch_layernorm(pre, p->norm2_w, p->norm2_b, out, (int64_t)B, E, p->ln_eps, pl.gemm[P_READOUT].ksplit, st);
}

}  // namespace wv
