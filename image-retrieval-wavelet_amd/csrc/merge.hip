// Merges of per-shard results of the sharded Hamming search for gfx950: sorted lists with their distance rows
// (k_merge_sorted), 16-bit lists with cumulative histograms (k_merge_cum), and relevance strings with cumulative histograms
// straight to average precision (k_merge_relbits_ap, k_merge_relbits_ap_cuts).  One workgroup (256 threads) merges one
// query; its dynamic LDS is MergeLayout's (merge.hpp).
#include "rank.hpp"
#include "merge.hpp"

namespace wv {

// ------------------------------------------------------------------------ merge of sorted shard lists
// Steps the three merge kernels share.  start[g][b] ([G][nbins + 1]) = first position of shard g's list with distance >= b.

// start[] from the shards' cumulative histograms (cum_ld: their row pitch in uint32): run boundaries are min(cum[b], kin)
__device__ __forceinline__ void merge_starts_from_cum(const uint32_t *__restrict__ cum, int64_t cum_ld, int G, int Q, int qi, int kin,
                                                      int nbins, int32_t *start, int tid)
{
    for (int u = tid; u < G * (nbins + 1); u += 256) {
        const int g = u / (nbins + 1), b = u - g * (nbins + 1);
        start[u] = (int32_t)min(cum[((int64_t)g * Q + qi) * cum_ld + b], (uint32_t)kin);
    }
}

// one wave: base[b] = entries of all shards with distance < b (totals per bin, then their exclusive scan)
__device__ __forceinline__ void merge_bin_bases(const int32_t *start, int G, int nbins, uint32_t *base, int lane)
{
    uint32_t t[3] = {0, 0, 0};
    const int b0 = 3 * lane;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (b0 + j < nbins)
            for (int g = 0; g < G; ++g) t[j] += (uint32_t)(start[g * (nbins + 1) + b0 + j + 1] - start[g * (nbins + 1) + b0 + j]);
    bin_scan3(t, nbins, base, lane);
}

// delta[g][b] ([G][nbins]): entry p of shard g, distance b, goes to output position p + delta[g][b]
__device__ __forceinline__ void merge_deltas(const int32_t *start, const uint32_t *base, int G, int nbins, int32_t *delta, int tid)
{
    for (int b = tid; b < nbins; b += 256) {
        uint32_t run = base[b];
        for (int g = 0; g < G; ++g) {
            const int s0 = start[g * (nbins + 1) + b], s1 = start[g * (nbins + 1) + b + 1];
            delta[g * nbins + b] = (int32_t)run - s0;
            run += (uint32_t)(s1 - s0);
        }
    }
}

// The G input lists of a query are each sorted by (distance, index) and come from contiguous row shards in
// rank order, so the merged order is: by distance bin, then by shard, then by position inside the shard's
// run of that distance.  Run boundaries come from binary searches on the sorted distance rows (no per-item
// histogram, no atomics); every entry's output position is  p + delta[g][d]  with one LDS lookup, entries are
// read in coalesced order and land in contiguous runs.
__global__ __launch_bounds__(256) void k_merge_sorted(const int32_t *__restrict__ idx_in,
                                                      const uint8_t *__restrict__ dist_in, int G, int Q, int kin,
                                                      int32_t *__restrict__ idx_out,
                                                      uint8_t *__restrict__ dist_out, int k, int nbins)
{
    extern __shared__ uint4 lds4[];
    const auto L = MergeLayout<int>::lists(G, nbins);
    int32_t *start = reinterpret_cast<int32_t *>(lds4) + L.start;
    int32_t *delta = reinterpret_cast<int32_t *>(lds4) + L.delta;
    uint32_t *base = reinterpret_cast<uint32_t *>(lds4) + L.base;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int64_t shard_stride = (int64_t)Q * kin;
    const uint8_t *dq = dist_in + (int64_t)qi * kin;
    const int32_t *iq = idx_in + (int64_t)qi * kin;

    for (int u = tid; u < G * (nbins + 1); u += 256) {
        const int g = u / (nbins + 1), b = u - g * (nbins + 1);
        const uint8_t *row = dq + g * shard_stride;
        int lo = 0, hi = kin;                                     // first p with row[p] >= b
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)row[mid] < b) lo = mid + 1;
            else hi = mid;
        }
        start[u] = lo;
    }
    __syncthreads();
    if (wv == 0) merge_bin_bases(start, G, nbins, base, lane);
    __syncthreads();
    merge_deltas(start, base, G, nbins, delta, tid);
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const uint8_t *row = dq + g * shard_stride;
        const int32_t *irow = iq + g * shard_stride;
        for (int p = tid; p < kin; p += 256) {
            const int d = row[p];
            if (d >= nbins) continue;                             // defensive: not a bin this call was sized for
            const int pos = p + delta[g * nbins + d];
            if (pos < k) {
                idx_out[(int64_t)qi * k + pos] = irow[p];
                if (dist_out) dist_out[(int64_t)qi * k + pos] = (uint8_t)d;
            }
        }
    }
}

// One wave: was every shard's prefix long enough for query qi?  T = the query's global k-th distance (first bin b with
// sum_g cum[g][b + 1] >= k, from the UNclamped histograms); shard g had to send cum[g][T + 1] entries.  The largest such
// count over all (shard, query) pairs of the launch goes to need_out: the exchange was exact iff it is <= the prefix sent
// (the caller clamps it to min(k, shard rows) first: with many ties at the k-th distance the raw count exceeds what a
// shard can owe).  cum_ld: row pitch of the histograms in uint32.
__device__ __forceinline__ void merge_report_need(const uint32_t *__restrict__ cum, int64_t cum_ld, int G, int Q, int qi, int nbins, int k,
                                                  int32_t *need_out, int lane)
{
    int T = nbins - 1;
    for (int c = 2; c >= 0; --c) {
        const int b = 64 * c + lane;
        uint32_t sb = 0;
        if (b < nbins)
            for (int g = 0; g < G; ++g) sb += cum[((int64_t)g * Q + qi) * cum_ld + b + 1];
        const uint64_t m = __ballot(b < nbins && sb >= (uint32_t)k);
        if (m) T = 64 * c + __builtin_ctzll(m);
    }
    uint32_t nd = 0;
    for (int g = lane; g < G; g += 64) nd = max(nd, cum[((int64_t)g * Q + qi) * cum_ld + T + 1]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) nd = max(nd, (uint32_t)__shfl_xor((int)nd, d, 64));
    if (lane == 0) atomicMax(need_out, (int32_t)min(nd, 0x7fffffffu));
}

// Compact form of the same merge for the sharded search: a shard does not send its distance rows (1 byte per
// entry) but its cumulative distance histogram (cum[b] = rows of the shard with distance < b, nbins + 1 words per
// query -- the k_hamming_topk by-product), and its list as 16-bit LOCAL row numbers (shards of <= 65536 rows).
// A sorted list is fully described by its histogram: run boundaries are min(cum[b], kin) directly, an entry's
// distance is the bin its position falls in (binary search over the boundaries in LDS), its global index is
// local + g * shard_rows.  Same output as k_merge_sorted on the expanded inputs.
__global__ __launch_bounds__(256) void k_merge_cum(const uint16_t *__restrict__ idx_local,
                                                   const uint32_t *__restrict__ cum, int G, int Q, int kin,
                                                   int64_t shard_rows, int32_t *__restrict__ idx_out,
                                                   uint8_t *__restrict__ dist_out, int k, int nbins,
                                                   int32_t *__restrict__ need_out)
{
    extern __shared__ uint4 lds4[];
    const auto L = MergeLayout<int>::lists(G, nbins);
    int32_t *start = reinterpret_cast<int32_t *>(lds4) + L.start;
    int32_t *delta = reinterpret_cast<int32_t *>(lds4) + L.delta;
    uint32_t *base = reinterpret_cast<uint32_t *>(lds4) + L.base;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    merge_starts_from_cum(cum, nbins + 1, G, Q, qi, kin, nbins, start, tid);
    __syncthreads();
    if (need_out && wv == 1) merge_report_need(cum, nbins + 1, G, Q, qi, nbins, k, need_out, lane);
    if (wv == 0) merge_bin_bases(start, G, nbins, base, lane);
    __syncthreads();
    merge_deltas(start, base, G, nbins, delta, tid);
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const uint16_t *irow = idx_local + ((int64_t)g * Q + qi) * kin;
        const int32_t *st = start + g * (nbins + 1);
        const int len = st[nbins];                                // entries this shard really sent
        for (int p = tid; p < len; p += 256) {
            int lo = 0, hi = nbins;                               // invariant: st[lo] <= p < st[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (st[mid] <= p) lo = mid;
                else hi = mid;
            }
            const int pos = p + delta[g * nbins + lo];
            if (pos < k) {
                idx_out[(int64_t)qi * k + pos] = (int32_t)((int64_t)irow[p] + g * shard_rows);
                if (dist_out) dist_out[(int64_t)qi * k + pos] = (uint8_t)lo;
            }
        }
    }
}

// ------------------------------------------------------------------------ merge of relevance strings
// Sharded mAP, receiving side: per query the G shards' relevance strings (bit p = is the shard's p-th nearest row relevant)
// and cumulative histograms -> average precision.  The global list orders entries by (distance, shard, position), so the
// merged relevance string is the concatenation, bin by bin and shard by shard, of runs of the shards' strings; it is
// assembled in LDS (k bits) with shifted 32-bit copies and walked exactly as a list is walked (ap_walk.hpp).
// need_out: as in k_merge_cum.

// Assembles the merged string of query blockIdx.x in LDS (L.string); ends with a workgroup barrier.
__device__ __forceinline__ void merge_relbits_string(uint32_t *lds, const MergeLayout<int> &L, const uint32_t *__restrict__ relbits,
                                                     const uint32_t *__restrict__ cum, int G, int Q, int kin, int w32, int k, int nbins,
                                                     int32_t *__restrict__ need_out, int64_t rb_ld32, int64_t cum_ld)
{
    int32_t *start = reinterpret_cast<int32_t *>(lds) + L.start;
    uint32_t *base = lds + L.base;
    uint32_t *M = lds + L.string;                                 // merged relevance string, k bits (+ spill word)
    const int mwords = L.string_words;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    merge_starts_from_cum(cum, cum_ld, G, Q, qi, kin, nbins, start, tid);
    for (int u = tid; u < mwords; u += 256) M[u] = 0;
    __syncthreads();
    if (need_out && wv == 1) merge_report_need(cum, cum_ld, G, Q, qi, nbins, k, need_out, lane);
    if (wv == 0) merge_bin_bases(start, G, nbins, base, lane);
    __syncthreads();
    for (int u = tid; u < G * nbins; u += 256) {                  // one run per (bin, shard)
        const int b = u / G, g = u - b * G;
        const int s0 = start[g * (nbins + 1) + b], n0 = start[g * (nbins + 1) + b + 1] - s0;
        if (n0 <= 0) continue;
        uint32_t dst = base[b];
        for (int g2 = 0; g2 < g; ++g2) dst += (uint32_t)(start[g2 * (nbins + 1) + b + 1] - start[g2 * (nbins + 1) + b]);
        if (dst >= (uint32_t)k) continue;
        const int n = min(n0, k - (int)dst);
        const uint32_t *src = relbits + ((int64_t)g * Q + qi) * rb_ld32;
        for (int o = 0; o < n; o += 32) {
            const int cnt = min(32, n - o), sp = s0 + o, sw = sp >> 5, sh = sp & 31;
            uint32_t v = src[sw] >> sh;
            if (sh && sw + 1 < w32) v |= src[sw + 1] << (32 - sh);
            if (cnt < 32) v &= (1u << cnt) - 1u;
            if (!v) continue;
            const uint32_t dp = dst + (uint32_t)o, dw = dp >> 5, ds = dp & 31;
            atomicOr(&M[dw], v << ds);
            if (ds && (v >> (32 - ds))) atomicOr(&M[dw + 1], v >> (32 - ds));
        }
    }
    __syncthreads();
}

// AP of the merged string at one cut-off k (wv_merge_relbits_map): the walk in chunks of ap_accum / ap_final.
// k_merge_relbits_ap_cuts below with one cut-off returns the same bits but was measured 19 - 29 % slower
// (profiles/list_ap_merge_refactor.txt), so this kernel stays; it is carved from the same layout (the walk's scratch is sized
// for the multi-cut form).
__global__ __launch_bounds__(256) void k_merge_relbits_ap(const uint32_t *__restrict__ relbits, const uint32_t *__restrict__ cum,
                                                          int G, int Q, int kin, int w32, int k, int nbins,
                                                          float *__restrict__ ap, int32_t *__restrict__ nrel,
                                                          int32_t *__restrict__ need_out, int64_t rb_ld32, int64_t cum_ld)
{
    extern __shared__ uint4 lds4[];
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds4);
    const auto L = MergeLayout<int>::relbits(G, nbins, k);
    merge_relbits_string(lds, L, relbits, cum, G, Q, kin, w32, k, nbins, need_out, rb_ld32, cum_ld);
    const uint32_t *M = lds + L.string;
    uint32_t *scratch = lds + L.scratch;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int R = (k + 255) / 256;
    double *wsum = reinterpret_cast<double *>(scratch + kApRounds * 4 + (kApRounds * 4 & 1));
    ApState st;
    for (int c0 = 0; c0 < R; c0 += kApRounds) {                   // chunks of 32 rounds: any k (mAP@ALL: k = database size)
        const int Rc = min(kApRounds, R - c0);
        uint32_t mine = 0;
        for (int r = 0; r < Rc; ++r) {
            const int p = (c0 + r) * 256 + tid;
            const bool rel = p < k && ((M[p >> 5] >> (p & 31)) & 1u);
            mine |= (rel ? 1u : 0u) << r;
            const uint64_t m = __ballot(rel);
            if (lane == 0) scratch[r * 4 + wv] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        ap_accum<256>(mine, scratch, Rc, c0, tid, st);
        __syncthreads();
    }
    ap_final<256>(st, wsum, tid, ap + qi, nrel ? nrel + qi : nullptr, [] { __syncthreads(); });
}

// The same at the cut-offs `cuts` (wv_merge_relbits_map_ks): the string is assembled for k = the largest, ap / nrel are
// [Q][cuts.n].
__global__ __launch_bounds__(256) void k_merge_relbits_ap_cuts(const uint32_t *__restrict__ relbits, const uint32_t *__restrict__ cum,
                                                               int G, int Q, int kin, int w32, int nbins, float *__restrict__ ap,
                                                               int32_t *__restrict__ nrel, int32_t *__restrict__ need_out,
                                                               int64_t rb_ld32, int64_t cum_ld, ApCuts cuts)
{
    extern __shared__ uint4 lds4[];
    const int k = cuts.k[cuts.n - 1], qi = blockIdx.x;
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds4);
    const auto L = MergeLayout<int>::relbits(G, nbins, k);
    merge_relbits_string(lds, L, relbits, cum, G, Q, kin, w32, k, nbins, need_out, rb_ld32, cum_ld);
    const uint32_t *M = lds + L.string;
    walk_cuts_256([M](int p) { return ((M[p >> 5] >> (p & 31)) & 1u) != 0; }, k, lds + L.scratch, cuts, ap + (int64_t)qi * cuts.n,
                  nrel ? nrel + (int64_t)qi * cuts.n : nullptr);
}

// THE gate of the merge launches: the layout must fit WV_MERGE_RELBITS_LDS_LIMIT.  A list merge (kmax = 0) has no fallback:
// WV_EINVAL; a string that does not fit (kmax = the largest cut-off) has one, the merged lists + wv_map_at_k[s]: WV_ENOTSUP.
static int merge_gate(const char *what, const MergeLayout<int64_t> &L, int G, int kmax)
{
    const size_t lds = L.bytes(), limit = WV_MERGE_RELBITS_LDS_LIMIT;
    if (lds <= limit) return WV_OK;
    if (kmax)
        WV_FAIL(WV_ENOTSUP, "%s: the merged string of the largest cut-off %d does not fit LDS beside the run boundaries "
                "of G=%d shards (%zu bytes needed, %zu available)", what, kmax, G, lds, limit);
    WV_FAIL(WV_EINVAL, "%s: the run boundaries of G=%d shards do not fit LDS (%zu bytes needed, %zu available)", what, G, lds, limit);
}

// What wv_merge_relbits_map and wv_merge_relbits_map_ks share: the argument rules, the gate and the launch geometry.  kmax: the
// (largest) cut-off; launch(lds bytes, relbits as dwords, w32, nbins, the two row pitches) starts the entry point's kernel.
template <typename LAUNCH>
static int merge_relbits(const char *what, const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q,
                         int kin, int kmax, int nbits, const float *ap, LAUNCH launch)
{
    WV_REQUIRE((relbits_ld == 0 || relbits_ld >= (kin + 63) / 64) && (cum_ld == 0 || cum_ld >= nbits + 2),
               "%s: row pitches %lld / %lld too small", what, (long long)relbits_ld, (long long)cum_ld);
    WV_REQUIRE(relbits && cum && ap, "%s: null buffer", what);
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1 && kmax >= 1, "%s: bad shape G=%d Q=%d kin=%d k=%d", what, G, Q, kin, kmax);
    if (int rc = require_nbits(what, nbits)) return rc;
    if (Q == 0) return WV_OK;
    const int nbins = nbits + 1, w32 = 2 * (int)ceil_div(kin, 64);
    const auto L = MergeLayout<int64_t>::relbits(G, nbins, kmax);
    if (int rc = merge_gate(what, L, G, kmax)) return rc;
    launch(L.bytes(), reinterpret_cast<const uint32_t *>(relbits), w32, nbins, relbits_ld ? 2 * relbits_ld : (int64_t)w32,
           cum_ld ? cum_ld : (int64_t)(nbins + 1));
    WV_CHECK_LAUNCH(what);
    return WV_OK;
}

}  // namespace wv

using namespace wv;

extern "C" int wv_topk_merge(const int32_t *idx_in, const uint8_t *dist_in, int G, int Q, int kin,
                             int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream)
{
    WV_REQUIRE(idx_in && dist_in && idx_out, "topk_merge: null buffer");
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1, "topk_merge: bad shape G=%d Q=%d kin=%d", G, Q, kin);
    if (int rc = require_nbits("topk_merge", nbits)) return rc;
    WV_REQUIRE(k >= 1 && (int64_t)k <= (int64_t)G * kin, "topk_merge: k=%d > G*kin", k);
    if (Q == 0) return WV_OK;
    const int nbins = nbits + 2;  // dist = nbits + 1 marks padding entries: they rank after every real one
    const auto L = MergeLayout<int64_t>::lists(G, nbins);
    if (int rc = merge_gate("topk_merge", L, G, 0)) return rc;
    hipLaunchKernelGGL(k_merge_sorted, dim3(Q), dim3(256), L.bytes(), (hipStream_t)stream, idx_in, dist_in, G, Q, kin,
                       idx_out, dist_out, k, nbins);
    WV_CHECK_LAUNCH("k_merge_sorted");
    return WV_OK;
}

extern "C" int wv_topk_merge_cum_need(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin, int64_t shard_rows,
                                      int32_t *idx_out, uint8_t *dist_out, int k, int nbits, int32_t *need_out, void *stream)
{
    WV_REQUIRE(idx_local && cum && idx_out, "topk_merge_cum: null buffer");
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1 && k >= 1, "topk_merge_cum: bad shape G=%d Q=%d kin=%d k=%d", G, Q, kin, k);
    if (int rc = require_nbits("topk_merge_cum", nbits)) return rc;
    WV_REQUIRE(shard_rows >= 1 && shard_rows <= 65536, "topk_merge_cum: %lld rows per shard do not fit 16-bit local indices",
               (long long)shard_rows);
    WV_REQUIRE((int64_t)G * shard_rows <= 0x7fffffffLL, "topk_merge_cum: indices exceed int32");
    if (Q == 0) return WV_OK;
    const int nbins = nbits + 1;
    const auto L = MergeLayout<int64_t>::lists(G, nbins);
    if (int rc = merge_gate("topk_merge_cum", L, G, 0)) return rc;
    hipLaunchKernelGGL(k_merge_cum, dim3(Q), dim3(256), L.bytes(), (hipStream_t)stream, idx_local, cum, G, Q, kin, shard_rows,
                       idx_out, dist_out, k, nbins, need_out);
    WV_CHECK_LAUNCH("k_merge_cum");
    return WV_OK;
}

extern "C" int wv_topk_merge_cum(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin,
                                 int64_t shard_rows, int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream)
{
    return wv_topk_merge_cum_need(idx_local, cum, G, Q, kin, shard_rows, idx_out, dist_out, k, nbits, nullptr, stream);
}

// ---------------------------------------------------------------------------------- sharded mAP, receiving side
extern "C" int wv_merge_relbits_map(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q,
                                    int kin, int k, int nbits, float *ap, int32_t *nrel, int32_t *need_out, void *stream)
{
    return merge_relbits("merge_relbits_map", relbits, relbits_ld, cum, cum_ld, G, Q, kin, k, nbits, ap,
                         [&](size_t lds, const uint32_t *rb32, int w32, int nbins, int64_t rb_ld32, int64_t cum_pitch) {
                             hipLaunchKernelGGL(k_merge_relbits_ap, dim3(Q), dim3(256), lds, (hipStream_t)stream, rb32, cum, G, Q, kin, w32,
                                                k, nbins, ap, nrel, need_out, rb_ld32, cum_pitch);
                         });
}

extern "C" int wv_merge_relbits_map_ks(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q,
                                       int kin, const int *ks, int nk, int nbits, float *ap, int32_t *nrel, int32_t *need_out,
                                       void *stream)
{
    ApCuts cuts;
    if (int rc = validate_cuts("merge_relbits_map_ks", ks, nk, 0x7fffffff, "INT_MAX", cuts)) return rc;
    return merge_relbits("merge_relbits_map_ks", relbits, relbits_ld, cum, cum_ld, G, Q, kin, cuts.k[nk - 1], nbits, ap,
                         [&](size_t lds, const uint32_t *rb32, int w32, int nbins, int64_t rb_ld32, int64_t cum_pitch) {
                             hipLaunchKernelGGL(k_merge_relbits_ap_cuts, dim3(Q), dim3(256), lds, (hipStream_t)stream, rb32, cum, G, Q, kin,
                                                w32, nbins, ap, nrel, need_out, rb_ld32, cum_pitch, cuts);
                         });
}

// dynamic LDS of k_merge_relbits_ap and k_merge_relbits_ap_cuts: one layout
extern "C" size_t wv_merge_relbits_map_ks_lds_bytes(int G, int kmax, int nbits)
{
    if (G < 1 || kmax < 1 || nbits < 1 || nbits > 128) return 0;
    return MergeLayout<int64_t>::relbits(G, nbits + 1, kmax).bytes();
}
