// Host twins of the head entry points ("wv_band_attn_pool ... _cpu twins of each taking host pointers"):
//   wv_band_attn_pool_cpu <- wv_band_attn_pool   CrossAttentionBottleneckHead*.forward in eval mode
//                                                (/root/reference/main/models/multi_dino_attention.py:1111-1141; :1030, :568, :448)
//   wv_band_attn_maps_cpu <- wv_band_attn_maps   what the head's nn.MultiheadAttention call returns (:1128), plus the scores
//   wv_hash_tail_cpu      <- wv_hash_tail        hash_fc -> BatchNorm1d(eval) -> sign (+ bit packing)  (:829-833)
//   wv_band_attn_pool_bf16_cpu <- wv_band_attn_pool_bf16   the same forward with both operands of the five dense weight
//                                                products rounded to bf16 (nearest even) and nothing else changed
// for a model whose tensors live on the host (module.to('cpu') -- explicit, never a silent fallback).
//
// fp32 throughout, like the kernels; every contraction is the same on any machine: eight interleaved fused-multiply-add
// chains (k mod 8) combined in one fixed tree -- the FMA instruction when the CPU has it, fmaf otherwise, the same bits.
// Against the GPU path the outputs agree to fp32 rounding (the kernels sum in MFMA order and use an erfc-polynomial GELU;
// tests hold both to the reference-made golden vectors with the same tolerance, 5e-5), the codes and packed words wherever
// |logit| exceeds that.  No HIP call, no thread, no global state.  Product code: shares nothing with oracle/.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "twin.hpp"
#include "head_args.hpp"

namespace {

constexpr int MB = 4;   // rows of x per pass over a weight row

inline float tree8(const float *a) { return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7])); }

// y[m][n] = bias[n] + sum_k x[m][k] w[n][k]   (x: M rows of pitch ldx, w: N rows of K, K % 8 == 0; y pitch ldy)
void linear_plain(const float *x, int64_t ldx, int M, const float *w, const float *bias, int N, int K, float *y, int64_t ldy)
{
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const float *xr = x + m * ldx, *wr = w + (int64_t)n * K;
            for (int k = 0; k < K; k += 8)
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(xr[k + j], wr[k + j], acc[j]);
            y[m * ldy + n] = tree8(acc) + (bias ? bias[n] : 0.f);
        }
}
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) void linear_fma(const float *x, int64_t ldx, int M, const float *w, const float *bias, int N,
                                                    int K, float *y, int64_t ldy)
{
    for (int m0 = 0; m0 < M; m0 += MB) {
        const int mb = M - m0 < MB ? M - m0 : MB;
        for (int n = 0; n < N; ++n) {
            __m256 acc[MB];
            for (int i = 0; i < MB; ++i) acc[i] = _mm256_setzero_ps();
            const float *wr = w + (int64_t)n * K;
            for (int k = 0; k < K; k += 8) {
                const __m256 wv = _mm256_loadu_ps(wr + k);
                for (int i = 0; i < mb; ++i) acc[i] = _mm256_fmadd_ps(_mm256_loadu_ps(x + (m0 + i) * ldx + k), wv, acc[i]);
            }
            for (int i = 0; i < mb; ++i) {
                float a[8];
                _mm256_storeu_ps(a, acc[i]);
                y[(m0 + i) * ldy + n] = tree8(a) + (bias ? bias[n] : 0.f);
            }
        }
    }
}
#endif
void linear(const float *x, int64_t ldx, int M, const float *w, const float *bias, int N, int K, float *y, int64_t ldy)
{
#if defined(__x86_64__)
    static const int has = (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) ? 1 : 0;
    if (has) return linear_fma(x, ldx, M, w, bias, N, K, y, ldy);
#endif
    linear_plain(x, ldx, M, w, bias, N, K, y, ldy);
}

void layer_norm(float *x, int E, const float *w, const float *b, float eps)
{
    double mean = 0.0, var = 0.0;
    for (int i = 0; i < E; ++i) mean += x[i];
    mean /= E;
    for (int i = 0; i < E; ++i) var += ((double)x[i] - mean) * ((double)x[i] - mean);
    const float inv = (float)(1.0 / sqrt(var / E + (double)eps)), mu = (float)mean;
    for (int i = 0; i < E; ++i) x[i] = (x[i] - mu) * inv * w[i] + b[i];
}

inline float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// bf16 value (round to nearest even) of an fp32 number, as an fp32 number
inline float bf16_round(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return f;   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}

std::vector<float> bf16_copy(const float *x, size_t n)
{
    std::vector<float> r(n);
    for (size_t i = 0; i < n; ++i) r[i] = bf16_round(x[i]);
    return r;
}

// The forward of both precisions.  bf16 = true: every operand of the five dense weight products is rounded to bf16 where it
// is read (weights once, up front); products of bf16 values are exact in fp32 and the accumulation is the fp32 chain of
// linear(), so nothing else changes.  what: the entry point's name in error texts.
int pool_cpu(const wv_head_params *p, const void *feats_any, int feat_dtype, int B, float *out, bool bf16, const char *what)
{
    WV_REQUIRE(p && feats_any && out, "%s: null buffer", what);
    const int E = p->embed_dim, H = p->num_heads, Nq = p->num_queries, S = p->num_tokens;
    WV_REQUIRE(E >= 8 && E % 8 == 0 && H >= 1 && E % H == 0 && Nq >= 1 && S >= 1 && S <= 64 && B >= 0,
               "%s: bad configuration E=%d heads=%d Nq=%d S=%d B=%d", what, E, H, Nq, S, B);
    WV_REQUIRE(p->q_eff && p->in_proj_w && p->in_proj_b && p->attn_out_w && p->attn_out_b && p->norm1_w && p->norm1_b &&
                   p->mlp0_w && p->mlp0_b && p->mlp2_w && p->mlp2_b && p->out_w && p->out_b && p->norm2_w && p->norm2_b,
               "%s: null parameter", what);
    if (B == 0) return WV_OK;
    const float *feats = feat_dtype == WV_DT_F32 ? static_cast<const float *>(feats_any) : nullptr;
    const uint16_t *feats16 = static_cast<const uint16_t *>(feats_any);
    const size_t ro_k = p->pool_mean ? (size_t)E : (size_t)Nq * E;
    std::vector<float> wkv_r, wo_r, w0_r, w2_r, wout_r, op;     // op: the rounded copy of an activation operand
    const float *wkv = p->in_proj_w + (size_t)E * E, *wo = p->attn_out_w, *w0 = p->mlp0_w, *w2 = p->mlp2_w, *wout = p->out_w;
    if (bf16) {
        wkv = (wkv_r = bf16_copy(wkv, (size_t)2 * E * E)).data();
        wo = (wo_r = bf16_copy(wo, (size_t)E * E)).data();
        w0 = (w0_r = bf16_copy(w0, (size_t)4 * E * E)).data();
        w2 = (w2_r = bf16_copy(w2, (size_t)4 * E * E)).data();
        wout = (wout_r = bf16_copy(wout, (size_t)E * ro_k)).data();
    }
    auto operand = [&](const std::vector<float> &x) {
        if (!bf16) return x.data();
        op.resize(x.size());
        for (size_t i = 0; i < x.size(); ++i) op[i] = bf16_round(x[i]);
        return (const float *)op.data();
    };
    const int d = E / H;
    const float scale = 1.f / sqrtf((float)d);
    // Q = q_eff Wq^T + bq: the query tokens are parameters, projected once (p->q_proj is a DEVICE pointer in the GPU path;
    // the host twin always projects)
    std::vector<float> Qp((size_t)Nq * E);
    linear(p->q_eff, E, Nq, p->in_proj_w, p->in_proj_b, E, E, Qp.data(), E);
    std::vector<float> kv((size_t)S * E), KV((size_t)S * 2 * E), ctx((size_t)Nq * E), x((size_t)Nq * E), hid((size_t)Nq * 4 * E),
        y((size_t)Nq * E), pooled((size_t)E);
    const int64_t sB = (int64_t)B * E;
    for (int b = 0; b < B; ++b) {
        for (int s = 0; s < S; ++s) {
            float *dst = kv.data() + (size_t)s * E;
            if (feats) {
                memcpy(dst, feats + s * sB + (int64_t)b * E, sizeof(float) * E);
            } else {
                const uint16_t *src = feats16 + s * sB + (int64_t)b * E;
                for (int i = 0; i < E; ++i) {
                    const uint32_t u = (uint32_t)src[i] << 16;
                    memcpy(dst + i, &u, 4);
                }
            }
        }
        // K | V = kv [Wk; Wv]^T + [bk; bv]  (rows E..3E of the packed in-projection)
        linear(operand(kv), E, S, wkv, p->in_proj_b + E, 2 * E, E, KV.data(), 2 * E);
        for (int h = 0; h < H; ++h)
            for (int nq = 0; nq < Nq; ++nq) {
                float sc[64], mx = -INFINITY;
                const float *qh = Qp.data() + (size_t)nq * E + h * d;
                for (int s = 0; s < S; ++s) {
                    const float *kh = KV.data() + (size_t)s * 2 * E + h * d;
                    float a = 0.f;
                    for (int j = 0; j < d; ++j) a = fmaf(qh[j], kh[j], a);
                    sc[s] = a * scale;
                    mx = fmaxf(mx, sc[s]);
                }
                float den = 0.f;
                for (int s = 0; s < S; ++s) { sc[s] = expf(sc[s] - mx); den += sc[s]; }
                float *o = ctx.data() + (size_t)nq * E + h * d;
                for (int j = 0; j < d; ++j) {
                    float a = 0.f;
                    for (int s = 0; s < S; ++s) a = fmaf(sc[s] / den, KV[(size_t)s * 2 * E + E + h * d + j], a);
                    o[j] = a;
                }
            }
        // x = LN1(q + attn.out_proj(ctx));  x = x + mlp.2(GELU(mlp.0(x)))
        linear(operand(ctx), E, Nq, wo, p->attn_out_b, E, E, x.data(), E);
        for (int nq = 0; nq < Nq; ++nq) {
            float *xr = x.data() + (size_t)nq * E;
            for (int i = 0; i < E; ++i) xr[i] += p->q_eff[(size_t)nq * E + i];
            layer_norm(xr, E, p->norm1_w, p->norm1_b, p->ln_eps);
        }
        linear(operand(x), E, Nq, w0, p->mlp0_b, 4 * E, E, hid.data(), 4 * E);
        for (size_t i = 0; i < hid.size(); ++i) hid[i] = gelu_erf(hid[i]);
        linear(operand(hid), 4 * E, Nq, w2, p->mlp2_b, E, 4 * E, y.data(), E);
        for (size_t i = 0; i < x.size(); ++i) x[i] += y[i];
        // read-out: mean over the queries then Linear(E -> E), or Linear(Nq E -> E) on the concatenation; LN2
        float *ob = out + (size_t)b * E;
        if (p->pool_mean) {
            for (int i = 0; i < E; ++i) {
                float a = 0.f;
                for (int nq = 0; nq < Nq; ++nq) a += x[(size_t)nq * E + i];
                pooled[(size_t)i] = a / (float)Nq;
            }
            linear(operand(pooled), E, 1, wout, p->out_b, E, E, ob, E);
        } else {
            linear(operand(x), (int64_t)Nq * E, 1, wout, p->out_b, E, Nq * E, ob, E);
        }
        layer_norm(ob, E, p->norm2_w, p->norm2_b, p->ln_eps);
    }
    return WV_OK;
}

// The attention call alone: scores, softmax per head, its mean over the heads, out_proj(context).  Same arithmetic and
// summation orders as pool_cpu above and as k_attn_maps: fmaf chain over the head dimension, x scale, max-subtracted expf,
// sum over the tokens in index order, one division; heads averaged in index order.
int maps_cpu(const wv_head_params *p, const float *feats, int layout, int B, float *probs, float *probs_mean, float *scores,
             float *attn_out)
{
    const int E = p->embed_dim, H = p->num_heads, Nq = p->num_queries, S = p->num_tokens, d = E / H;
    const float scale = 1.f / sqrtf((float)d), inv_heads = 1.f / (float)H;
    const int ldkv = attn_out ? 2 * E : E;                      // K alone when nothing needs V
    std::vector<float> Qp((size_t)Nq * E), kv((size_t)S * E), KV((size_t)S * ldkv), P((size_t)H * Nq * S), ctx((size_t)Nq * E);
    linear(p->q_eff, E, Nq, p->in_proj_w, p->in_proj_b, E, E, Qp.data(), E);
    for (int b = 0; b < B; ++b) {
        for (int s = 0; s < S; ++s) {
            const size_t row = layout == WV_TOKENS_BSE ? (size_t)b * S + s : (size_t)s * B + b;
            memcpy(kv.data() + (size_t)s * E, feats + row * E, sizeof(float) * E);
        }
        linear(kv.data(), E, S, p->in_proj_w + (size_t)E * E, p->in_proj_b + E, ldkv, E, KV.data(), ldkv);
        for (int h = 0; h < H; ++h)
            for (int nq = 0; nq < Nq; ++nq) {
                float *pr = P.data() + ((size_t)h * Nq + nq) * S, mx = -INFINITY;
                const float *qh = Qp.data() + (size_t)nq * E + h * d;
                for (int s = 0; s < S; ++s) {
                    const float *kh = KV.data() + (size_t)s * ldkv + h * d;
                    float a = 0.f;
                    for (int j = 0; j < d; ++j) a = fmaf(qh[j], kh[j], a);
                    pr[s] = a * scale;
                    mx = fmaxf(mx, pr[s]);
                }
                if (scores) memcpy(scores + (((size_t)b * H + h) * Nq + nq) * S, pr, sizeof(float) * S);
                float den = 0.f;
                for (int s = 0; s < S; ++s) { pr[s] = expf(pr[s] - mx); den += pr[s]; }
                for (int s = 0; s < S; ++s) pr[s] = pr[s] / den;
            }
        if (probs) memcpy(probs + (size_t)b * H * Nq * S, P.data(), sizeof(float) * P.size());
        if (probs_mean)
            for (int i = 0; i < Nq * S; ++i) {
                float a = 0.f;
                for (int h = 0; h < H; ++h) a += P[(size_t)h * Nq * S + i];
                probs_mean[(size_t)b * Nq * S + i] = a * inv_heads;
            }
        if (attn_out) {
            for (int nq = 0; nq < Nq; ++nq)
                for (int e = 0; e < E; ++e) {
                    const float *pr = P.data() + ((size_t)(e / d) * Nq + nq) * S;
                    float a = 0.f;
                    for (int s = 0; s < S; ++s) a = fmaf(pr[s], KV[(size_t)s * ldkv + E + e], a);
                    ctx[(size_t)nq * E + e] = a;
                }
            linear(ctx.data(), E, Nq, p->attn_out_w, p->attn_out_b, E, E, attn_out + (size_t)b * Nq * E, E);
        }
    }
    return WV_OK;
}

}  // namespace

extern "C" int wv_band_attn_maps_cpu(const wv_head_params *p, const float *feats, int layout, int B, float *probs, float *probs_mean,
                                     float *scores, float *attn_out)
{
    char why[256];
    if (const int rc = ::wv::head_attn_args_refusal(p, B, "band_attn_maps_cpu", why, sizeof(why))) WV_FAIL(rc, "%s", why);
    WV_REQUIRE(probs || probs_mean || scores || attn_out, "band_attn_maps_cpu: no output asked for");
    WV_REQUIRE(layout == WV_TOKENS_SBE || layout == WV_TOKENS_BSE, "band_attn_maps_cpu: layout=%d (WV_TOKENS_SBE or WV_TOKENS_BSE)",
               layout);
    if (B == 0) return WV_OK;
    WV_REQUIRE(feats, "band_attn_maps_cpu: null buffer");
    return maps_cpu(p, feats, layout, B, probs, probs_mean, scores, attn_out);
}

extern "C" int wv_band_attn_pool_cpu(const wv_head_params *p, const float *feats, int B, float *out)
{
    return pool_cpu(p, feats, WV_DT_F32, B, out, false, "band_attn_pool_cpu");
}

extern "C" int wv_band_attn_pool_bf16_cpu(const wv_head_params *p, const void *feats, int feat_dtype, int B, float *out)
{
    WV_REQUIRE(feat_dtype == WV_DT_F32 || feat_dtype == WV_DT_BF16, "band_attn_pool_bf16_cpu: feat_dtype=%d (WV_DT_F32 or WV_DT_BF16)",
               feat_dtype);
    WV_REQUIRE(!p || p->embed_dim % 32 == 0, "band_attn_pool_bf16_cpu: embed_dim=%d must be a multiple of 32", p->embed_dim);
    return pool_cpu(p, feats, feat_dtype, B, out, true, "band_attn_pool_bf16_cpu");
}

extern "C" int wv_hash_tail_cpu(const float *fused, int B, int E, const float *hash_w, const float *hash_b, const float *bn_w,
                                const float *bn_b, const float *bn_mean, const float *bn_var, float bn_eps, int nbits,
                                float *logits_out, float *codes_out, uint64_t *packed_out)
{
    WV_REQUIRE(fused && hash_w, "hash_tail_cpu: null buffer");
    WV_REQUIRE(B >= 0 && E >= 8 && E % 8 == 0 && nbits >= 1, "hash_tail_cpu: bad shape B=%d E=%d nbits=%d", B, E, nbits);
    WV_REQUIRE(!bn_w || (bn_b && bn_mean && bn_var), "hash_tail_cpu: incomplete BatchNorm parameters");
    const int words = (nbits + 63) / 64;
    std::vector<float> logit((size_t)nbits);
    for (int b = 0; b < B; ++b) {
        linear(fused + (size_t)b * E, E, 1, hash_w, hash_b, nbits, E, logit.data(), nbits);
        if (packed_out) memset(packed_out + (size_t)b * words, 0, sizeof(uint64_t) * words);
        for (int j = 0; j < nbits; ++j) {
            float v = logit[(size_t)j];
            if (bn_w) v = (v - bn_mean[j]) / sqrtf(bn_var[j] + bn_eps) * bn_w[j] + bn_b[j];
            if (logits_out) logits_out[(size_t)b * nbits + j] = v;
            if (codes_out) codes_out[(size_t)b * nbits + j] = v > 0.f ? 1.f : (v < 0.f ? -1.f : (v == 0.f ? 0.f : v));
            if (packed_out && v > 0.f) packed_out[(size_t)b * words + j / 64] |= 1ull << (j % 64);
        }
    }
    return WV_OK;
}
