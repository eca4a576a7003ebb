// Attention maps of the band-attention head: what nn.MultiheadAttention returns for the head's attention call
// (the reference's main/models/multi_dino_attention.py:1128) -- out_proj(context), the softmax probabilities per head or
// averaged over the heads -- and the scaled scores in front of the softmax, as outputs of their own.  The head's forward
// (wv_band_attn_pool) keeps these values in LDS only; this is the diagnostic path that writes them out, for hooks on
// `head.attn` and for studies of the attention itself.  Same stages as the separate launches of head.hip: query projection,
// K | V in-projection on the fp32 matrix-core GEMM gemm_f32 picks, one VALU kernel per sample with k_attn_core's arithmetic
// in k_attn_core's order, out-projection GEMM.  Nothing wv_band_attn_pool launches is touched.
#include "head.hpp"

namespace wv {

// One workgroup per sample.
//   Qp   [Nq][E]          projected queries (batch-invariant)
//   KV   [S*B][ldkv]      K (ldkv = E) or K | V (ldkv = 2E) of every token; token s of sample b is row s*B + b
//                         (WV_TOKENS_SBE) or b*S + s (WV_TOKENS_BSE)
//   scores, probs [B][heads][Nq][S], probs_mean [B][Nq][S], ctx [B*Nq][E] (needs V): each optional
__global__ __launch_bounds__(256) void k_attn_maps(const float *__restrict__ Qp, const float *__restrict__ KV, int ldkv,
                                                   int layout, float *__restrict__ scores, float *__restrict__ probs,
                                                   float *__restrict__ probs_mean, float *__restrict__ ctx, int B, int E,
                                                   int heads, int Nq, int S)
{
    // LDS: kv[S][ldkv + 4] (rows padded by 16 bytes, as in k_attn_core) | q[Nq][E] | P[Nq][heads][S]
    extern __shared__ float4 msm4[];
    float *kv = reinterpret_cast<float *>(msm4);
    const int KP = ldkv + 4;
    float *q = kv + (size_t)S * KP;
    float *P = q + (size_t)Nq * E;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hd = E / heads;
    const float scale = 1.0f / sqrtf((float)hd);
    const int row4 = ldkv / 4;
    for (int t = tid; t < S * row4; t += blockDim.x) {
        const int s = t / row4, c = t - s * row4;
        const size_t row = layout == WV_TOKENS_BSE ? (size_t)b * S + s : (size_t)s * B + b;
        *reinterpret_cast<float4 *>(kv + (size_t)s * KP + 4 * c) = *reinterpret_cast<const float4 *>(KV + row * ldkv + 4 * c);
    }
    for (int t = tid; t < Nq * E / 4; t += blockDim.x)
        *reinterpret_cast<float4 *>(q + 4 * t) = *reinterpret_cast<const float4 *>(Qp + 4 * t);
    __syncthreads();
    const int ndots = Nq * heads * S;
    for (int t = tid; t < ndots; t += blockDim.x) {
        const int s = t % S, hh = (t / S) % heads, i = t / (S * heads);
        const float *qv = q + (size_t)i * E + hh * hd;
        const float *kr = kv + (size_t)s * KP + hh * hd;
        float acc = 0.f;
        for (int d = 0; d < hd; ++d) acc = fmaf(qv[d], kr[d], acc);
        P[t] = acc * scale;
    }
    __syncthreads();
    // P is [Nq][heads][S], the outputs are [heads][Nq][S]: consecutive threads write consecutive output elements
    auto store_per_head = [&](float *dst) {
        for (int o = tid; o < ndots; o += blockDim.x) {
            const int s = o % S, i = (o / S) % Nq, hh = o / (S * Nq);
            dst[(size_t)b * ndots + o] = P[((size_t)i * heads + hh) * S + s];
        }
    };
    if (scores) {
        store_per_head(scores);
        __syncthreads();   // the softmax below overwrites P
    }
    for (int t = tid; t < Nq * heads; t += blockDim.x) {
        float *p = P + (size_t)t * S;
        float mx = p[0];
        for (int s = 1; s < S; ++s) mx = fmaxf(mx, p[s]);
        float sum = 0.f;
        for (int s = 0; s < S; ++s) {
            p[s] = expf(p[s] - mx);
            sum += p[s];
        }
        for (int s = 0; s < S; ++s) p[s] = p[s] / sum;
    }
    __syncthreads();
    if (probs) store_per_head(probs);
    if (probs_mean) {
        const float inv = 1.0f / (float)heads;
        for (int o = tid; o < Nq * S; o += blockDim.x) {
            const int s = o % S, i = o / S;
            float sum = 0.f;
            for (int hh = 0; hh < heads; ++hh) sum += P[((size_t)i * heads + hh) * S + s];
            probs_mean[(size_t)b * Nq * S + o] = sum * inv;
        }
    }
    if (ctx) {   // the host passes it only with ldkv = 2E: V is columns E .. 2E of a row
        for (int t = tid; t < Nq * E; t += blockDim.x) {
            const int e = t % E, i = t / E, hh = e / hd;
            const float *p = P + ((size_t)i * heads + hh) * S;
            float acc = 0.f;
            for (int s = 0; s < S; ++s) acc = fmaf(p[s], kv[(size_t)s * KP + E + e], acc);
            ctx[((size_t)b * Nq + i) * E + e] = acc;
        }
    }
}

}  // namespace wv

using namespace wv;

extern "C" size_t wv_band_attn_maps_workspace_bytes(const wv_head_params *p, int B)
{
    return p && B > 0 ? head_maps_ws_layout(p, B).bytes : 0;
}

extern "C" int wv_band_attn_maps(const wv_head_params *p, const float *feats, int layout, int B, float *probs, float *probs_mean,
                                 float *scores, float *attn_out, void *workspace, size_t workspace_bytes, void *stream)
{
    char why[256];
    if (const int rc = head_attn_args_refusal(p, B, "band_attn_maps", why, sizeof(why))) WV_FAIL(rc, "%s", why);
    WV_REQUIRE(probs || probs_mean || scores || attn_out, "band_attn_maps: no output asked for");
    WV_REQUIRE(layout == WV_TOKENS_SBE || layout == WV_TOKENS_BSE, "band_attn_maps: layout=%d (WV_TOKENS_SBE or WV_TOKENS_BSE)",
               layout);
    const int E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    if (head_attn_lds_bytes(p) > (size_t)kMaxLdsBytes)
        WV_FAIL(WV_ENOTSUP, "band_attn_maps: %d tokens x %d queries at embed_dim=%d do not fit the attention kernel's LDS", S, Nq, E);
    WV_REQUIRE((int64_t)B * std::max(Nq, S) < (1ll << 31), "band_attn_maps: B=%d too large", B);
    if (B == 0) return WV_OK;
    WV_REQUIRE(feats, "band_attn_maps: null buffer");
    const HeadMapsWs ws = head_maps_ws_layout(p, B);
    WV_REQUIRE(workspace && workspace_bytes >= ws.bytes, "band_attn_maps: workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
    hipStream_t st = (hipStream_t)stream;
    const float *Qp = p->q_proj;
    if (!Qp) {
        launch_qproj(p, ws_at<float>(workspace, ws.Qp), st);
        Qp = ws_at<float>(workspace, ws.Qp);
    }
    // K | V of all S*B tokens, row = the token's row in the caller's layout: rows E..3E of in_proj_weight; K alone (rows
    // E..2E) when nothing needs V
    const int ldkv = attn_out ? 2 * E : E;
    const char *pin = ::wv::tune("WV_GEMM");
    float *KV = ws_at<float>(workspace, ws.KV), *ctx = attn_out ? ws_at<float>(workspace, ws.ctx) : nullptr;
    launch_gemm_f32({gemm_f32((int64_t)S * B, ldkv, E, pin), 1}, feats, p->in_proj_w + (size_t)E * E, p->in_proj_b + E, KV, S * B, ldkv,
                    E, st);
    const size_t lds = ((size_t)S * (ldkv + 4) + (size_t)Nq * E + (size_t)Nq * p->num_heads * S) * sizeof(float);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_attn_maps), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_attn_maps, dim3(B), dim3(256), lds, st, Qp, KV, ldkv, layout, scores, probs, probs_mean, ctx, B, E,
                       p->num_heads, Nq, S);
    if (attn_out)   // output[0] of the module: out_proj(context) + bias
        launch_gemm_f32({gemm_f32((int64_t)B * Nq, E, E, pin), 1}, ctx, p->attn_out_w, p->attn_out_b, attn_out, B * Nq, E, E, st);
    WV_CHECK_LAUNCH("band_attn_maps");
    return WV_OK;
}
