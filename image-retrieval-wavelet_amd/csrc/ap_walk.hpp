// Average precision from relevance bits in list order -- the arithmetic and summation order of wv_map_at_k, stated
// independently by its host twin (host_rank.cpp): position p = round * TPQ + t, the j-th hit adds the fp32 quotient
// j / (p + 1) to a double, threads summed per wave, waves in index order.  Shared by the fused ranking + AP kernel
// (rank2.hip), the batch mAP proxy (ip_map.hip), the merge of per-shard relevance strings (merge.hip) and the AP of
// written lists (list_ap.hip).
#pragma once
#include "common.hpp"
#include "ap_cuts.hpp"

namespace wv {

constexpr int kApRounds = 32;                // list positions per thread kept as bits at a time (one chunk of the walk)

// dwords of LDS scratch the walk needs: hit counts [kApRounds][NW] + NW doubles (8-byte aligned)
template <int TPQ>
__host__ __device__ constexpr int ap_scratch_dwords() { return kApRounds * (TPQ / 64) + 2 * (TPQ / 64) + 2; }

// The walk comes in chunks of up to kApRounds rounds, so that lists of any length go through the same arithmetic:
//   ApState st;  for every chunk { lane 0 of every wave writes cnt[r_local * NW + wave] = hits of that wave in the round;
//                                  group barrier;  ap_accum(relbits, cnt, rounds, first round, t, st);  group barrier; }
//   ap_final(st, ...).
// A thread's quotients are added to its double in increasing list position whatever the chunking: the result does not
// depend on it, bit for bit.
struct ApState {
    uint32_t running = 0;    // hits before the current round, all threads
    double acc = 0.0;        // this thread's sum of fp32 quotients j / rank
};

// relbits: bit r = relevance of position (r_base + r) * TPQ + t (r < Rc <= 32); cnt[r * NW + wave] as above, already published.
template <int TPQ>
__device__ __forceinline__ void ap_accum(uint32_t relbits, const uint32_t *cnt, int Rc, int r_base, int t, ApState &st)
{
    constexpr int NW = TPQ / 64, CH = 8;
    const int wv = t >> 6;
    for (int r0 = 0; r0 < Rc; r0 += CH) {
        uint32_t c[CH][NW];
#pragma unroll
        for (int u = 0; u < CH; ++u)
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) c[u][w2] = cnt[min(r0 + u, Rc - 1) * NW + w2];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int r = r0 + u;
            if (r < Rc) {                                         // uniform
                uint32_t before = st.running, tot = 0;
#pragma unroll
                for (int w2 = 0; w2 < NW; ++w2) {
                    before += w2 < wv ? c[u][w2] : 0u;
                    tot += c[u][w2];
                }
                const bool rel = (relbits >> r) & 1u;
                const uint64_t m = __ballot(rel);
                if (rel) {
                    const uint32_t j = before + (uint32_t)mbcnt(m) + 1;
                    st.acc += (double)((float)j / (float)((r_base + r) * TPQ + t + 1));
                }
                st.running += tot;
            }
        }
    }
}

// wsum: NW doubles of LDS (8-byte aligned) that nothing else uses until the second barrier
template <int TPQ, typename SYNC>
__device__ __forceinline__ void ap_final(const ApState &st, double *wsum, int t, float *__restrict__ ap_out,
                                         int32_t *__restrict__ nrel_out, SYNC group_barrier)
{
    constexpr int NW = TPQ / 64;
    const int lane = t & 63, wv = t >> 6;
    const double acc = wave_sum_f64(st.acc);
    if (lane == 0) wsum[wv] = acc;
    group_barrier();
    if (t == 0) {
        double s = wsum[0];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) s += wsum[w2];
        *ap_out = st.running ? (float)(s / (double)st.running) : 0.0f;
        if (nrel_out) *nrel_out = (int32_t)st.running;
    }
}

// ---- several cut-offs from one walk (wv_hamming_map_at_ks, wv_merge_relbits_map_ks, wv_map_at_ks).
// List position p = round * TPQ + t does not depend on k, a thread adds its quotients in increasing position, and the list
// for the largest cut-off has the list for every smaller one as a prefix (the order distance, then row is total): AP@c is
// a snapshot of the walk to k_max, taken in the round that holds position c - 1, with the bits of a walk to c.
// ApCuts and the rule for its contents: ap_cuts.hpp.

// dwords of LDS scratch of the multi-cut walk: the single-cut walk's + the waves' hit counts below a cut
template <int TPQ>
__host__ __device__ constexpr int ap_cuts_scratch_dwords() { return ap_scratch_dwords<TPQ>() + TPQ / 64; }

// ap_accum for a chunk of the walk to cuts.k[cuts.n - 1], writing ap_out[i] / nrel_out[i] (or NULL) for every cut i whose
// last position lies in the chunk.  `next`: the first cut not written yet (0 before the first chunk); after the last chunk
// every cut is written, ap_final is not called.  In the round of a cut c a thread with p < c contributes
// st.acc + its own quotient, every other thread st.acc alone; the hits of the round with p < c come from a masked ballot
// (cnt holds whole rounds).  Each snapshot takes ap_final's way: wave butterfly, waves in index order.
// wsum: NW doubles (8-byte aligned), wcut: NW dwords, both free LDS.  Control flow is uniform over the TPQ threads.
template <int TPQ, typename SYNC>
__device__ __forceinline__ void ap_accum_cuts(uint32_t relbits, const uint32_t *cnt, int Rc, int r_base, int t, ApState &st,
                                              const ApCuts &cuts, int &next, double *wsum, uint32_t *wcut,
                                              float *__restrict__ ap_out, int32_t *__restrict__ nrel_out, SYNC group_barrier)
{
    constexpr int NW = TPQ / 64, CH = 8;
    const int lane = t & 63, wv = t >> 6;
    // the next cut-off in a register: read from the kernel arguments when it changes, not in every round
    int64_t cut = next < cuts.n ? cuts.k[next] : INT64_MAX;
    for (int r0 = 0; r0 < Rc; r0 += CH) {
        uint32_t c[CH][NW];
#pragma unroll
        for (int u = 0; u < CH; ++u)
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) c[u][w2] = cnt[min(r0 + u, Rc - 1) * NW + w2];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int r = r0 + u;
            if (r < Rc) {                                         // uniform
                uint32_t before = st.running, tot = 0;
#pragma unroll
                for (int w2 = 0; w2 < NW; ++w2) {
                    before += w2 < wv ? c[u][w2] : 0u;
                    tot += c[u][w2];
                }
                const bool rel = (relbits >> r) & 1u;
                const uint64_t m = __ballot(rel);
                const int p = (r_base + r) * TPQ + t;
                double own = 0.0;                                 // this thread's quotient of the round
                if (rel) {
                    const uint32_t j = before + (uint32_t)mbcnt(m) + 1;
                    own = (double)((float)j / (float)(p + 1));
                }
                // cuts whose last position c - 1 lies in this round (uniform; several may share a round)
                while (cut <= (int64_t)(r_base + r + 1) * TPQ) {
                    const bool in = rel && p < cut;
                    const uint64_t mc = __ballot(in);
                    const double acc = wave_sum_f64(in ? st.acc + own : st.acc);
                    if (lane == 0) {
                        wsum[wv] = acc;
                        wcut[wv] = (uint32_t)__popcll(mc);
                    }
                    group_barrier();
                    if (t == 0) {
                        double s = wsum[0];
                        uint32_t running = st.running + wcut[0];
#pragma unroll
                        for (int w2 = 1; w2 < NW; ++w2) {
                            s += wsum[w2];
                            running += wcut[w2];
                        }
                        ap_out[next] = running ? (float)(s / (double)running) : 0.0f;
                        if (nrel_out) nrel_out[next] = (int32_t)running;
                    }
                    group_barrier();                              // wsum / wcut are free for the next cut
                    ++next;
                    cut = next < cuts.n ? cuts.k[next] : INT64_MAX;
                }
                if (rel) st.acc += own;
                st.running += tot;
            }
        }
    }
}

// The whole walk of a 256-thread workgroup that owns one query, at the cut-offs `cuts`: what the multi-cut merge of relevance
// strings (k_merge_relbits_ap_cuts, merge.hip) and the multi-cut AP over written lists (k_map_at_ks, list_ap.hip) share.  rel_at(p) = relevance of list
// position p < k (free of side effects: the last position is asked again for the padding of the last round); scratch:
// ap_cuts_scratch_dwords<256>() dwords of LDS, 8-byte aligned; ap / nrel: the query's rows of cuts.n entries.
template <typename REL>
__device__ __forceinline__ void walk_cuts_256(REL rel_at, int k, uint32_t *scratch, const ApCuts &cuts, float *__restrict__ ap,
                                              int32_t *__restrict__ nrel)
{
    constexpr int CH = 8;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int R = (k + 255) / 256;
    double *wsum = reinterpret_cast<double *>(scratch + kApRounds * 4 + (kApRounds * 4 & 1));
    uint32_t *wcut = reinterpret_cast<uint32_t *>(wsum + 4);
    ApState st;
    int next = 0;
    for (int c0 = 0; c0 < R; c0 += kApRounds) {                   // chunks of 32 rounds: any k (mAP@ALL: k = database size)
        const int Rc = min(kApRounds, R - c0);
        uint32_t mine = 0;
        for (int r0 = 0; r0 < Rc; r0 += CH) {                     // a batch's reads are issued before the first is used
            bool rv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) rv[u] = rel_at(min((c0 + r0 + u) * 256 + tid, k - 1));
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int r = r0 + u;
                const bool rel = r < Rc && (c0 + r) * 256 + tid < k && rv[u];
                mine |= (rel ? 1u : 0u) << (r & 31);
                const uint64_t m = __ballot(rel);
                if (lane == 0 && r < Rc) scratch[r * 4 + wv] = (uint32_t)__popcll(m);
            }
        }
        __syncthreads();
        ap_accum_cuts<256>(mine, scratch, Rc, c0, tid, st, cuts, next, wsum, wcut, ap, nrel, [] { __syncthreads(); });
        __syncthreads();
    }
}

}  // namespace wv
