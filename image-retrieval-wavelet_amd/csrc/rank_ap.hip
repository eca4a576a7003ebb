// Rank-approximation AP losses for gfx950: SmoothAP and SupAP (main/losses/smooth_rank_ap.py), AP per query row and its
// gradient w.r.t. the row's scores.  Nothing of size B x M x M exists; the definitions, the per-pair term, the limits and the
// argument rules are rank_ap.hpp's and include/wvhash.h's.
//
// k_rank_ap_pack: one wave per 64 columns of a row, T != 0 by ballot -> the bit rows of T [B][W], bits past M clear.
// k_rank_ap_lm (quick form): one wave per 64 columns j of row i, LM[i][j] = (bit row i AND bit row j) != 0, by ballot.
// k_rank_ap_rows: workgroup q of 512 threads (8 waves) owns query row q.
//   stage    S[q,:] and the row's bit words into LDS; wave 0 scans the words' popcounts (DPP), then every thread places
//            its set columns: the positives' list, ascending, so the slot of a positive is a popcount below it.
//   pass A   wave v takes positives v, v + 8, ...: lanes stride j (the 64 lanes of step k share bit word k: one broadcast
//            read; S[j] by consecutive lanes), each lane sums R, R w, R', R' w of its columns, xor shuffles add the lanes,
//            lane 0 leaves the positive's record (f, 1 / (rk n), its own gradient entry).  Quick form: word k of T[i] and
//            LM[i] comes from the workspace, one address per wave.
//   AP       the records' f: per thread, per wave by xor shuffles, the 8 waves in index order.
//   pass B   (grad wanted) thread t owns columns j = t, t + 512, ...: it walks the positives in list order (list, score and
//            record are broadcast reads), evaluates R'(S[j] - S[i]) again and adds g_ij; a positive column subtracts its
//            record's own entry.  One writer per gradient element: no atomics, one order for every sum.
// Same bits from run to run.
#include "common.hpp"
#include "rank_ap.hpp"

namespace wv {

constexpr int kRaThreads = 512;
constexpr int kRaWaves = kRaThreads / kWave;
constexpr int kRaPackWaves = 4;

// sT [W] u64 | rec [M] | sS [M] | wpre [kRankApMaxWords + 1] | red [kRaWaves] | pos [M] u16
inline size_t rank_ap_lds(int M)
{
    return (size_t)rank_ap_words(M) * sizeof(uint64_t) + (size_t)M * (sizeof(RankApRecord) + sizeof(float) + sizeof(uint16_t)) +
           (kRankApMaxWords + 1 + kRaWaves) * sizeof(float);
}
static_assert(sizeof(RankApRecord) == 12 && kRankApMax <= 65536, "record of three floats; a column index fits 16 bits");
static_assert(kRankApMaxWords <= kWave, "one wave scans the popcounts of a bit row");

__global__ __launch_bounds__(kRaPackWaves *kWave) void k_rank_ap_pack(const float *__restrict__ T, int M, int W,
                                                                       uint64_t *__restrict__ bits)
{
    const int q = blockIdx.y, k = blockIdx.x * kRaPackWaves + wave_id(), j = k * 64 + lane_id();
    if (k >= W) return;                                  // wave-uniform
    const bool set = j < M && T[(int64_t)q * M + j] != 0.f;
    const uint64_t word = __ballot(set);
    if (lane_id() == 0) bits[(int64_t)q * W + k] = word;
}

__global__ __launch_bounds__(kWave) void k_rank_ap_lm(const uint64_t *__restrict__ bits, int B, int W,
                                                      uint64_t *__restrict__ lm)
{
    const int i = blockIdx.y, k = blockIdx.x, j = k * 64 + lane_id();
    bool hit = false;
    if (j < B)
        for (int w = 0; w < W; ++w) hit |= (bits[(int64_t)i * W + w] & bits[(int64_t)j * W + w]) != 0;
    const uint64_t word = __ballot(hit);
    if (lane_id() == 0) lm[(int64_t)i * W + k] = word;
}

__global__ __launch_bounds__(kRaThreads) void k_rank_ap_rows(const float *__restrict__ S, const uint64_t *__restrict__ Tb,
                                                             const uint64_t *__restrict__ LM, int M, int W,
                                                             wv_rank_ap_params p, float *__restrict__ ap,
                                                             float *__restrict__ grad)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint64_t *sT = reinterpret_cast<uint64_t *>(lds);             // [W]
    RankApRecord *rec = reinterpret_cast<RankApRecord *>(sT + W); // [M], the first np used
    float *sS = reinterpret_cast<float *>(rec + M);               // [M]
    int *wpre = reinterpret_cast<int *>(sS + M);                  // positives before word k; [kRankApMaxWords]: all
    float *red = reinterpret_cast<float *>(wpre + kRankApMaxWords + 1);
    uint16_t *pos = reinterpret_cast<uint16_t *>(red + kRaWaves); // [M], the first np used

    const int q = blockIdx.x, t = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool quick = p.form == WV_RANK_AP_QUICK, want_grad = grad != nullptr;

    for (int j = t; j < M; j += kRaThreads) sS[j] = S[(int64_t)q * M + j];
    if (t < W) sT[t] = Tb[(int64_t)q * W + t];
    __syncthreads();
    if (wave == 0) {
        const uint32_t c = lane < W ? (uint32_t)__builtin_popcountll(sT[lane]) : 0u;
        const uint32_t inc = wave_incl_scan_u32(c);
        if (lane < W) wpre[lane] = (int)(inc - c);
        if (lane == kWave - 1) wpre[kRankApMaxWords] = (int)inc;
    }
    __syncthreads();
    const int np = wpre[kRankApMaxWords];
    for (int j = t; j < M; j += kRaThreads) {
        const uint64_t w = sT[j >> 6];
        const int b = j & 63;
        if ((w >> b) & 1) pos[wpre[j >> 6] + __builtin_popcountll(w & ((1ull << b) - 1))] = (uint16_t)j;
    }
    __syncthreads();

    for (int pi = wave; pi < np; pi += kRaWaves) {
        const int i = pos[pi];
        const float si = sS[i];
        float sR = 0.f, sRw = 0.f, sD = 0.f, sDw = 0.f;
        for (int k = 0; k < W; ++k) {
            const int j = k * 64 + lane;
            const uint64_t tq = sT[k];
            const uint64_t ww = quick ? Tb[(int64_t)i * W + k] : tq;
            const uint64_t tw = quick ? (LM[(int64_t)i * W + k] & tq) : tq;
            if (j < M && j != i) {
                const RankTerm r = rank_term(p, sS[j] - si, (tw >> lane) & 1);
                const bool w = (ww >> lane) & 1;
                sR += r.R, sRw += w ? r.R : 0.f;
                if (want_grad) sD += r.dR, sDw += w ? r.dR : 0.f;
            }
        }
        sR = wave_sum_f32(sR), sRw = wave_sum_f32(sRw);
        if (want_grad) sD = wave_sum_f32(sD), sDw = wave_sum_f32(sDw);
        if (lane == 0) rec[pi] = rank_ap_record(sR, sRw, sD, sDw, np);
    }
    __syncthreads();

    float s = 0.f;
    for (int pi = t; pi < np; pi += kRaThreads) s += rec[pi].f;
    s = wave_sum_f32(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (t == 0) {
        float a = 0.f;
        for (int w = 0; w < kRaWaves; ++w) a += red[w];
        ap[q] = np > 0 ? a / (float)np : 0.f;
    }
    if (!want_grad) return;

    for (int j = t; j < M; j += kRaThreads) {
        const int k = j >> 6, b = j & 63;
        const uint64_t tq = sT[k];
        const bool tqj = (tq >> b) & 1;
        const float sj = sS[j];
        float acc = 0.f;
        // SupAP, general form, positive column: every pair is a target pair, derivative 0
        if (!(p.kind == WV_RANK_AP_SUP && !quick && tqj)) {
            for (int pi = 0; pi < np; ++pi) {
                const int i = pos[pi];
                if (i == j) continue;
                bool w = tqj, tgt = tqj;
                if (quick) {
                    w = (Tb[(int64_t)i * W + k] >> b) & 1;
                    tgt = tqj && ((LM[(int64_t)i * W + k] >> b) & 1);
                }
                const RankTerm r = rank_term(p, sj - sS[i], tgt);
                acc += rank_ap_coeff(rec[pi], w, r.dR);
            }
        }
        if (tqj) acc -= rec[wpre[k] + __builtin_popcountll(tq & ((1ull << b) - 1))].own;
        grad[(int64_t)q * M + j] = acc;
    }
}

}  // namespace wv

extern "C" size_t wv_rank_ap_workspace_bytes(int B, int M, int form) { return wv::rank_ap_ws_bytes(B, M, form); }

extern "C" int wv_rank_ap(const float *scores, const float *target, int B, int M, const wv_rank_ap_params *p, float *ap,
                          float *grad, void *ws, size_t ws_bytes, void *stream)
{
    const int refused = wv::rank_ap_args("rank_ap", scores, target, B, M, p, ap, true, ws, ws_bytes);
    if (refused != WV_OK) return refused;
    const int W = wv::rank_ap_words(M);
    const bool quick = p->form == WV_RANK_AP_QUICK;
    uint64_t *bits = static_cast<uint64_t *>(ws);
    uint64_t *lm = quick ? bits + (size_t)B * W : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wv::k_rank_ap_pack, dim3((unsigned)((W + wv::kRaPackWaves - 1) / wv::kRaPackWaves), (unsigned)B),
                       dim3(wv::kRaPackWaves * wv::kWave), 0, st, target, M, W, bits);
    WV_CHECK_LAUNCH("rank_ap (pack)");
    if (quick) {
        hipLaunchKernelGGL(wv::k_rank_ap_lm, dim3((unsigned)W, (unsigned)B), dim3(wv::kWave), 0, st, bits, B, W, lm);
        WV_CHECK_LAUNCH("rank_ap (label matrix)");
    }
    const size_t lds = wv::rank_ap_lds(M);
    if (int rc = wv::set_lds_attr(reinterpret_cast<const void *>(wv::k_rank_ap_rows), lds, "rank_ap")) return rc;
    hipLaunchKernelGGL(wv::k_rank_ap_rows, dim3((unsigned)B), dim3(wv::kRaThreads), lds, st, scores, bits, lm, M, W, *p, ap,
                       grad);
    WV_CHECK_LAUNCH("rank_ap");
    return WV_OK;
}
