// Pairwise hashing losses for gfx950: SCHLoss (main/losses/dsch.py:31-59) and HashNetLoss (main/losses/hashnet_loss.py:49-66),
// value and gradient w.r.t. the embeddings in two launches; the B x B matrices (Gram, relation, bounds, weights, per-pair
// terms) exist only in registers and LDS.  The per-pair term, the limits and the argument rules are pair_loss.hpp's.
//
// k_pair_main: workgroup b of 256 threads owns rows i in [8 b, 8 b + 8) and walks all columns j in tiles of 32.
//   stage    u_i (once) and the tile's u_j into LDS, squashed while staged (tanh(pre_scale * e)); row pitch D | 1 (odd).
//   pairs    thread t has pair (r = t / 32, c = t % 32): G as four interleaved fmaf chains over k.  The 32 lanes of a half
//            wave read ONE u_i address (broadcast) and 32 u_j rows an odd pitch apart: conflict-free ds_read_b32.  Then
//            pair_term() on the popcounts of the label words; v1, v2 and the positive count stay in the thread's registers
//            across the tiles, a1, a2 go to LDS as [c][r].
//   gradient (grad wanted) thread t owns columns d = t, t + 256 of the 8 rows:  g_p[r][d] += a_p[c][r] * u_j[c][d]  over the
//            tile's c -- the coefficients are broadcast ds_read_b128, u_j[c][d] is one row read by consecutive lanes.
//   end      g1, g2 of the 8 rows to the workspace (no other workgroup writes them: no atomics), and the workgroup's sums
//            in one PairLossPartial record: wave sums by xor shuffles, then the four waves in index order.
// k_pair_finish: every workgroup adds the records in the same fixed tree (bit-identical scalars in all of them), forms
//   pair_loss_scalars(), workgroup 0 writes out[3], and all write grad = (kappa1 g1 + kappa2 g2) * chain(u) elementwise.
// Same bits from run to run: no floating-point atomics, every sum has one order.
#include "common.hpp"
#include "pair_loss.hpp"

namespace wv {

constexpr int kPlThreads = 256;
constexpr int kPlSlots = kPairLossMaxD / kPlThreads;      // columns d a thread owns in the gradient step
static_assert(kPlRows * kPlCols == kPlThreads, "one pair per thread");
// a1, a2, the wave sums of v1 / v2 and of the positive count; u_i and u_j follow
constexpr size_t kPlFixedLds = 2 * kPlThreads * sizeof(float) + 2 * (kPlThreads / 64) * sizeof(double) + (kPlThreads / 64) * sizeof(uint32_t);
static_assert(kPlFixedLds % 16 == 0, "u_i starts on a 16-byte boundary");
inline size_t pair_main_lds(int D) { return kPlFixedLds + (size_t)(kPlRows + kPlCols) * (D | 1) * sizeof(float); }
static_assert(kPairLossMaxD % kPlThreads == 0 && kPlRows % 4 == 0, "whole slots, float4 coefficient reads");
static_assert((kPairLossMaxRows + kPlRows - 1) / kPlRows <= kPlThreads, "the finishing tree takes one record per thread");

__global__ __launch_bounds__(kPlThreads) void k_pair_main(const float *__restrict__ e, const uint64_t *__restrict__ lab,
                                                          int lwords, int B, int D, wv_pair_loss_params p,
                                                          float *__restrict__ g, PairLossPartial *__restrict__ part,
                                                          int want_grad)
{
    // one dynamic region, 16-byte aligned, the float4-read coefficients first: no static LDS shifts its base
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float *a1 = reinterpret_cast<float *>(lds);        // [kPlCols][kPlRows]
    float *a2 = a1 + kPlThreads;
    double *red = reinterpret_cast<double *>(a2 + kPlThreads);
    uint32_t *redn = reinterpret_cast<uint32_t *>(red + 2 * (kPlThreads / 64));
    const int pitch = D | 1;
    float *ui = reinterpret_cast<float *>(lds + kPlFixedLds);   // [kPlRows][pitch]
    float *uj = ui + kPlRows * pitch;                  // [kPlCols][pitch]

    const int t = threadIdx.x, r = t / kPlCols, c = t % kPlCols;
    const int i0 = blockIdx.x * kPlRows, i = i0 + r;

    for (int x = t; x < kPlRows * D; x += kPlThreads) {
        const int rr = x / D, d = x - rr * D;
        ui[rr * pitch + d] = i0 + rr < B ? pl_squash(p, e[(int64_t)(i0 + rr) * D + d]) : 0.f;
    }
    uint64_t li0 = 0, li1 = 0;
    if (i < B) {
        li0 = lab[(int64_t)i * lwords];
        if (lwords == 2) li1 = lab[(int64_t)i * lwords + 1];
    }
    const int ni = pl_popc(li0) + pl_popc(li1);

    float acc1[kPlRows][kPlSlots], acc2[kPlRows][kPlSlots];
#pragma unroll
    for (int rr = 0; rr < kPlRows; ++rr)
#pragma unroll
        for (int s = 0; s < kPlSlots; ++s) acc1[rr][s] = acc2[rr][s] = 0.f;
    float s1 = 0.f, s2 = 0.f;
    uint32_t n1 = 0;

    for (int j0 = 0; j0 < B; j0 += kPlCols) {
        __syncthreads();                               // the previous tile is read (first pass: nothing to wait for)
        for (int x = t; x < kPlCols * D; x += kPlThreads) {
            const int cc = x / D, d = x - cc * D;
            uj[cc * pitch + d] = j0 + cc < B ? pl_squash(p, e[(int64_t)(j0 + cc) * D + d]) : 0.f;
        }
        __syncthreads();
        const int j = j0 + c;
        PairTerm pt = {0.f, 0.f, 0.f, 0.f, 0};
        if (i < B && j < B) {
            const float *a = ui + r * pitch, *b = uj + c * pitch;
            float G0 = 0.f, G1 = 0.f, G2 = 0.f, G3 = 0.f;
            int k = 0;
            for (; k + 4 <= D; k += 4) {
                G0 = fmaf(a[k], b[k], G0);
                G1 = fmaf(a[k + 1], b[k + 1], G1);
                G2 = fmaf(a[k + 2], b[k + 2], G2);
                G3 = fmaf(a[k + 3], b[k + 3], G3);
            }
            for (; k < D; ++k) G0 = fmaf(a[k], b[k], G0);
            const uint64_t lj0 = lab[(int64_t)j * lwords], lj1 = lwords == 2 ? lab[(int64_t)j * lwords + 1] : 0ull;
            pt = pair_term(p, (G0 + G1) + (G2 + G3), ni, pl_popc(lj0) + pl_popc(lj1), pl_popc(li0 & lj0) + pl_popc(li1 & lj1));
            s1 += pt.v1, s2 += pt.v2, n1 += (uint32_t)pt.pos;
        }
        if (want_grad) {                               // uniform
            a1[c * kPlRows + r] = pt.a1;               // pairs outside the batch: 0
            a2[c * kPlRows + r] = pt.a2;
            __syncthreads();
            const int nc = min(kPlCols, B - j0);
#pragma unroll
            for (int s = 0; s < kPlSlots; ++s) {
                const int d = s * kPlThreads + t;
                if (d < D) {
                    for (int cc = 0; cc < nc; ++cc) {
                        const float u = uj[cc * pitch + d];
#pragma unroll
                        for (int q = 0; q < kPlRows; q += 4) {
                            const float4 x1 = *reinterpret_cast<const float4 *>(a1 + cc * kPlRows + q);
                            const float4 x2 = *reinterpret_cast<const float4 *>(a2 + cc * kPlRows + q);
                            acc1[q][s] = fmaf(x1.x, u, acc1[q][s]);
                            acc1[q + 1][s] = fmaf(x1.y, u, acc1[q + 1][s]);
                            acc1[q + 2][s] = fmaf(x1.z, u, acc1[q + 2][s]);
                            acc1[q + 3][s] = fmaf(x1.w, u, acc1[q + 3][s]);
                            acc2[q][s] = fmaf(x2.x, u, acc2[q][s]);
                            acc2[q + 1][s] = fmaf(x2.y, u, acc2[q + 1][s]);
                            acc2[q + 2][s] = fmaf(x2.z, u, acc2[q + 2][s]);
                            acc2[q + 3][s] = fmaf(x2.w, u, acc2[q + 3][s]);
                        }
                    }
                }
            }
        }
    }

    if (want_grad) {
        float *g1 = g, *g2 = g + (int64_t)B * D;
#pragma unroll
        for (int s = 0; s < kPlSlots; ++s) {
            const int d = s * kPlThreads + t;
            if (d < D) {
#pragma unroll
                for (int rr = 0; rr < kPlRows; ++rr)
                    if (i0 + rr < B) {
                        g1[(int64_t)(i0 + rr) * D + d] = acc1[rr][s];
                        g2[(int64_t)(i0 + rr) * D + d] = acc2[rr][s];
                    }
            }
        }
    }

    const double w1 = wave_sum_f64((double)s1), w2 = wave_sum_f64((double)s2);
    const uint32_t wn = wave_sum_u32(n1);
    if (lane_id() == 0) red[2 * wave_id()] = w1, red[2 * wave_id() + 1] = w2, redn[wave_id()] = wn;
    __syncthreads();
    if (t == 0) {
        PairLossPartial o = {0., 0., 0, 0};
        for (int w = 0; w < kPlThreads / 64; ++w) o.s1 += red[2 * w], o.s2 += red[2 * w + 1], o.n1 += redn[w];
        part[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pair_finish(const float *__restrict__ e, int B, int D, wv_pair_loss_params p,
                                                            const float *__restrict__ g,
                                                            const PairLossPartial *__restrict__ part, int nparts,
                                                            float *__restrict__ out, float *__restrict__ grad)
{
    __shared__ double t1[kPlThreads], t2[kPlThreads];
    __shared__ unsigned long long tn[kPlThreads];
    const int t = threadIdx.x;
    t1[t] = t < nparts ? part[t].s1 : 0.;
    t2[t] = t < nparts ? part[t].s2 : 0.;
    tn[t] = t < nparts ? part[t].n1 : 0ull;
    for (int h = kPlThreads / 2; h > 0; h >>= 1) {     // one tree, the same in every workgroup
        __syncthreads();
        if (t < h) t1[t] += t1[t + h], t2[t] += t2[t + h], tn[t] += tn[t + h];
    }
    __syncthreads();
    const PairLossScalars sc = pair_loss_scalars(p, B, t1[0], t2[0], tn[0]);
    if (blockIdx.x == 0 && t == 0) out[0] = sc.loss, out[1] = sc.part1, out[2] = sc.part2;
    if (!grad) return;
    const int64_t n = (int64_t)B * D, x = (int64_t)blockIdx.x * kPlThreads + t;
    if (x < n) {
        const float u = pl_squash(p, e[x]);
        grad[x] = fmaf(sc.kappa1, g[x], sc.kappa2 * g[n + x]) * pl_chain(p, u);
    }
}

}  // namespace wv

extern "C" size_t wv_pair_loss_workspace_bytes(int B, int D) { return wv::pair_loss_ws_bytes(B, D); }

extern "C" int wv_pair_loss(const float *e, const uint64_t *labels, int lwords, int B, int D, const wv_pair_loss_params *p,
                            float *out, float *grad, void *ws, size_t ws_bytes, void *stream)
{
    const int refused = wv::pair_loss_args("pair_loss", e, labels, lwords, B, D, p, out, true, ws, ws_bytes);
    if (refused != WV_OK) return refused;
    const int nb = wv::pair_loss_blocks(B);
    float *g = static_cast<float *>(ws);
    auto *part = reinterpret_cast<wv::PairLossPartial *>(static_cast<char *>(ws) + wv::pair_loss_g_bytes(B, D));
    const size_t lds = wv::pair_main_lds(D);
    if (int rc = wv::set_lds_attr(reinterpret_cast<const void *>(wv::k_pair_main), lds, "pair_loss")) return rc;
    hipLaunchKernelGGL(wv::k_pair_main, dim3((unsigned)nb), dim3(wv::kPlThreads), lds, (hipStream_t)stream, e, labels, lwords, B,
                       D, *p, g, part, grad ? 1 : 0);
    WV_CHECK_LAUNCH("pair_loss");
    const int64_t n = (int64_t)B * D;
    const unsigned fin = grad ? (unsigned)((n + wv::kPlThreads - 1) / wv::kPlThreads) : 1u;
    hipLaunchKernelGGL(wv::k_pair_finish, dim3(fin), dim3(wv::kPlThreads), 0, (hipStream_t)stream, e, B, D, *p, g, part, nb, out,
                       grad);
    WV_CHECK_LAUNCH("pair_loss (finish)");
    return WV_OK;
}
