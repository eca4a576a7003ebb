// NDCG from graded label overlap (DSCH/_utils.py:551-574): rel(q, n) = popcount(qlab[q] & dblab[n]), gain 2^rel - 1.
//   k_label_overlap_hist  per query, how many rows share exactly r classes with it (r = 0 .. 64 * lwords): all the ideal DCG
//                         needs of the N gains -- no [Q][N] matrix, no sort
//   k_ndcg_at_ks          DCG and ideal DCG of a ranked list at several cut-offs from one walk
// Host twins: host_ndcg.cpp (same integers; DCG / IDCG bit for bit, see the summation order below).
#include "common.hpp"
#include "ap_walk.hpp"
#include "ndcg.hpp"

namespace wv {

// ------------------------------------------------------------------------------------------------- overlap histogram
// One workgroup = kOvQT queries x a slice of kOvRows rows.  A thread holds the label words of one row per step (loaded once,
// reused for the kOvQT queries, whose words are wave-uniform scalar loads).  Counting, per query and 64 rows: most rows share
// nothing with the query, so one LDS add per row would put nearly every lane on bin 0 or 1; instead the wave loops over the
// DISTINCT overlaps present (first live lane's r -> ballot(r == r0) -> lane 0 adds the popcount to the wave's PRIVATE row of
// the table), typically 2..4 turns.  One lane per wave and address: no contended atomic.  The waves' rows are summed at the
// end and added to hist (zeroed on the stream by the entry point) with one global add per non-empty bin.
constexpr int kOvQT = 16;
constexpr int kOvRows = 4096;

template <int LW>
__global__ __launch_bounds__(256) void k_label_overlap_hist(const uint64_t *__restrict__ qlab, const uint64_t *__restrict__ dblab,
                                                            int Q, int64_t N, uint32_t *__restrict__ hist)
{
    constexpr int BINS = 64 * LW + 1;
    __shared__ uint32_t tab[4 * kOvQT * BINS];
    const int tid = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(wave_id());
    const int q0 = blockIdx.y * kOvQT, nq = min(kOvQT, Q - q0);
    const int64_t n0 = (int64_t)blockIdx.x * kOvRows, n1 = min(N, n0 + kOvRows);
    for (int e = tid; e < 4 * kOvQT * BINS; e += 256) tab[e] = 0;
    __syncthreads();
    uint32_t *mine = tab + wave * (kOvQT * BINS);
    for (int64_t base = n0; base < n1; base += 256) {             // uniform trip count
        const int64_t n = base + tid;
        const bool valid = n < n1;                                // a tail row is counted nowhere
        uint64_t row[LW];
#pragma unroll
        for (int w = 0; w < LW; ++w) row[w] = valid ? dblab[n * LW + w] : 0ull;
        const uint64_t live = __ballot(valid);
        for (int j = 0; j < nq; ++j) {
            const uint64_t *ql = qlab + (int64_t)(q0 + j) * LW;   // uniform address
            int r = 0;
#pragma unroll
            for (int w = 0; w < LW; ++w) r += __popcll(row[w] & ql[w]);
            uint64_t todo = live;
            while (todo) {                                        // uniform: one turn per distinct overlap among the live lanes
                const int r0 = __builtin_amdgcn_readlane(r, __builtin_ctzll(todo));
                const uint64_t m = __ballot(valid && r == r0);
                if (lane == 0) atomicAdd(&mine[j * BINS + r0], (uint32_t)__popcll(m));
                todo &= ~m;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nq * BINS; e += 256) {
        const uint32_t s = tab[e] + tab[kOvQT * BINS + e] + tab[2 * kOvQT * BINS + e] + tab[3 * kOvQT * BINS + e];
        if (s) atomicAdd(&hist[(int64_t)q0 * BINS + e], s);
    }
}

// ------------------------------------------------------------------------------------------------- DCG / ideal DCG walk
// One query per 256-thread workgroup.  Summation order (ap_walk.hpp's scheme with two fp64 accumulators, shared with
// wv_ndcg_at_ks_cpu): position p = round * 256 + t; a thread adds its terms in increasing position with an explicit
// fma(gain, w[p], acc); a cut-off c is a snapshot in the round that holds position c - 1 -- threads with p < c contribute
// their fma, the others their acc --, reduced by the wave butterfly (wave_sum_f64), then the waves in index order.
// Ideal term of position p: the largest r with #{rows with rel >= r} > p, found by a bit-descent over the descending
// cumulative table in LDS (padded with zeros to 2 * 64 * LW entries, so that no probe needs a bound); never a difference of
// prefix sums.  No fp64 division, no transcendental: w is the host-made table of wv_ndcg_weights.
template <int LW>
__global__ __launch_bounds__(256) void k_ndcg_at_ks(const int32_t *__restrict__ idx, int64_t ld, const uint64_t *__restrict__ qlab,
                                                    const uint64_t *__restrict__ dblab, const uint32_t *__restrict__ hist,
                                                    const double *__restrict__ w, double *__restrict__ dcg,
                                                    double *__restrict__ idcg, ApCuts cuts)
{
    constexpr int B = 64 * LW, BINS = B + 1, TAB = 2 * B;
    __shared__ uint32_t h[BINS];
    __shared__ uint32_t ge[TAB];                                  // ge[r] = rows with rel >= r (1 <= r <= B), 0 elsewhere
    __shared__ double wsum[8];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int qi = blockIdx.x, k = cuts.k[cuts.n - 1];
    const int32_t *list = idx + (int64_t)qi * ld;
    uint64_t qreg[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) qreg[i] = qlab[(int64_t)qi * LW + i];
    if (tid < BINS) h[tid] = hist[(int64_t)qi * BINS + tid];
    __syncthreads();
    if (tid < TAB) {
        uint32_t s = 0;
        if (tid >= 1)
            for (int b = tid; b <= B; ++b) s += h[b];
        ge[tid] = s;
    }
    __syncthreads();

    double accd = 0.0, acci = 0.0;
    int next = 0;
    int64_t cut = cuts.k[0];
    const int R = (k + 255) / 256;
    for (int r = 0; r < R; ++r) {
        const int p = r * 256 + tid;
        const bool active = p < k;
        const int32_t id = active ? list[p] : -1;
        const double wp = active ? w[p] : 0.0;                    // a position past the walk adds 0 to both sums
        int rel = 0;
        if (id >= 0) {                                            // an absent entry (< 0) contributes 0, as in k_map_at_ks
            const uint64_t *dl = dblab + (int64_t)id * LW;
#pragma unroll
            for (int i = 0; i < LW; ++i) rel += __popcll(dl[i] & qreg[i]);
        }
        int best = 0;
#pragma unroll
        for (int s = B; s >= 1; s >>= 1)
            if (ge[best + s] > (uint32_t)p) best += s;
        const double newd = fma(ndcg_gain(rel), wp, accd);
        const double newi = fma(ndcg_gain(best), wp, acci);
        while (cut <= (int64_t)(r + 1) * 256) {                   // cuts whose last position lies in this round (uniform)
            const bool in = p < cut;
            const double sd = wave_sum_f64(in ? newd : accd);
            const double si = wave_sum_f64(in ? newi : acci);
            if (lane == 0) {
                wsum[wv] = sd;
                wsum[4 + wv] = si;
            }
            __syncthreads();
            if (tid == 0) {
                dcg[(int64_t)qi * cuts.n + next] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
                idcg[(int64_t)qi * cuts.n + next] = wsum[4] + wsum[5] + wsum[6] + wsum[7];
            }
            __syncthreads();                                      // wsum is free for the next cut
            ++next;
            cut = next < cuts.n ? cuts.k[next] : INT64_MAX;
        }
        accd = newd;
        acci = newi;
    }
}

}  // namespace wv

using namespace wv;

extern "C" int wv_label_overlap_hist(const uint64_t *qlab, const uint64_t *dblab, int lwords, int Q, int64_t N, uint32_t *hist,
                                     void *stream)
{
    if (int rc = ndcg_hist_args("label_overlap_hist", qlab && dblab && hist, lwords, Q, N)) return rc;
    if (Q == 0) return WV_OK;
    const int64_t qtiles = ceil_div(Q, kOvQT);
    if (qtiles > 65535) WV_FAIL(WV_ENOTSUP, "label_overlap_hist: %d queries in one call (at most %d)", Q, 65535 * kOvQT);
    const dim3 grid((unsigned)ceil_div(N, kOvRows), (unsigned)qtiles);      // N < 2^32: at most 2^20 slices
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)Q * (64 * lwords + 1), st);
    if (e != hipSuccess) WV_FAIL(WV_EHIP, "label_overlap_hist: memset: %s", hipGetErrorString(e));
    if (lwords == 1)
        hipLaunchKernelGGL((k_label_overlap_hist<1>), grid, dim3(256), 0, st, qlab, dblab, Q, N, hist);
    else
        hipLaunchKernelGGL((k_label_overlap_hist<2>), grid, dim3(256), 0, st, qlab, dblab, Q, N, hist);
    WV_CHECK_LAUNCH("k_label_overlap_hist");
    return WV_OK;
}

extern "C" int wv_ndcg_at_ks(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                             int lwords, const uint32_t *hist, const double *w, double *dcg, double *idcg, void *stream)
{
    static_assert(kMaxCutoffs == WV_MAX_CUTOFFS, "ap_walk.hpp and wvhash.h disagree");
    if (int rc = ndcg_walk_args("ndcg_at_ks", idx && qlab && dblab && hist && w && dcg && idcg, ld, Q, ks, nk, lwords)) return rc;
    if (Q == 0) return WV_OK;
    ApCuts cuts;                                                  // by value in the kernel arguments
    cuts.n = nk;
    for (int i = 0; i < kMaxCutoffs; ++i) cuts.k[i] = i < nk ? ks[i] : 0;
    hipStream_t st = (hipStream_t)stream;
    if (lwords == 1)
        hipLaunchKernelGGL((k_ndcg_at_ks<1>), dim3(Q), dim3(256), 0, st, idx, ld, qlab, dblab, hist, w, dcg, idcg, cuts);
    else
        hipLaunchKernelGGL((k_ndcg_at_ks<2>), dim3(Q), dim3(256), 0, st, idx, ld, qlab, dblab, hist, w, dcg, idcg, cuts);
    WV_CHECK_LAUNCH("k_ndcg_at_ks");
    return WV_OK;
}
