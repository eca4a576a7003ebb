// Fused Hamming distance + stable top-k ranking, list merge and average precision for gfx950.
//
// Reference: per query  hamm = 0.5*(B - q @ r.T); indices = torch.argsort(hamm)[:topk]
// (accuracy_calculator.py:219-223) -- an O(N log N) comparison sort of a key with only B+1
// distinct values.  Here: an exact counting sort in O(N), ties broken by ascending database
// index (= torch.argsort(stable=True)).
//
// One workgroup (256 threads) ranks one query.  Thread t owns the CONTIGUOUS item range
// [t*C, (t+1)*C), C = ceil(N/256), and a private column hist[bin][t] of an LDS table, so that
//   phase 1  hist[d][t] += 1                     (conflict-free: bank = t mod 32 for every bin)
//   scan     offs[d][t] = sum_{b<d} tot[b] + sum_{t'<t} hist[d][t']   (exclusive, bin-major)
//   phase 2  pos = offs[d][t]++  -> idx[pos] = item      (only for d <= threshold bin T)
// reproduces the stable order with no atomics, no sort and no inter-lane matching.  The
// database is pre-transposed once per call into dbT[r][t] = code[t*C + r] so that the
// per-thread contiguous ranges are read with fully coalesced loads.  The distance row is not
// scattered at all: it is regenerated from the bin boundaries (sorted => run-length).
//
// This is the column kernel: it takes any N and any k.  Databases (shards) of at most 32,768 rows go to the windowed
// kernel (rank2.hip); rank_plan() (rank.hpp) decides which.  The file also holds the ranking entry points, the merges
// of sorted shard lists and the AP kernels over written lists.
#include "rank.hpp"
#include "ap_walk.hpp"

namespace wv {

// ------------------------------------------------------------------------ item sources
// CodeSource: items are database codes, distance = popcount(q ^ code), id = row + offset
template <int WORDS>
struct CodeSource {
    const uint64_t *dbT;  // [C][256][WORDS]
    uint64_t qw[WORDS];
    int64_t idx_offset;
    struct Raw {
        uint64_t w[WORDS];
    };
    __device__ __forceinline__ Raw fetch(int r, int t, int64_t) const
    {
        const uint64_t *p = dbT + ((int64_t)r * kTopkThreads + t) * WORDS;
        Raw c;
        if constexpr (WORDS == 2) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            c.w[0] = (uint64_t)v.x | ((uint64_t)v.y << 32);
            c.w[1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
        } else {
#pragma unroll
            for (int w = 0; w < WORDS; ++w) c.w[w] = p[w];
        }
        return c;
    }
    __device__ __forceinline__ int dist(const Raw &c) const
    {
        int d = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) d += __popcll(c.w[w] ^ qw[w]);
        return d;
    }
    __device__ __forceinline__ int32_t id(int64_t item) const { return (int32_t)(item + idx_offset); }
};

// RowSource: items are the entries of one stored distance-matrix row
struct RowSource {
    const uint8_t *row;
    int64_t n;
    using Raw = int;
    __device__ __forceinline__ Raw fetch(int, int, int64_t item) const { return item < n ? row[item] : 0; }
    __device__ __forceinline__ int dist(const Raw &c) const { return c; }
    __device__ __forceinline__ int32_t id(int64_t item) const { return (int32_t)item; }
};

// Exclusive scan over the bins of per-bin totals held 3 bins per lane of one wave (lane l: bins 3l .. 3l + 2; 192 >=
// kMaxBins): base[b] = sum of the bins below b.  Returns the sum of the bins below the lane's first.
__device__ __forceinline__ uint32_t bin_scan3(const uint32_t (&t)[3], int nbins, uint32_t *base, int lane)
{
    const int b0 = 3 * lane;
    const uint32_t incl = wave_incl_scan_u32(t[0] + t[1] + t[2]);
    const uint32_t excl = incl - (t[0] + t[1] + t[2]);
    if (b0 < nbins) base[b0] = excl;
    if (b0 + 1 < nbins) base[b0 + 1] = excl + t[0];
    if (b0 + 2 < nbins) base[b0 + 2] = excl + t[0] + t[1];
    return excl;
}

// ------------------------------------------------------------------------ the ranking core
// LDS: hist[nbins][256] (u32, or u16 pairs when n_items < 65536), tot[kMaxBins], base[kMaxBins + 1], misc
//
// U16 = true packs two threads' counters into one dword (thread t uses half t & 1 of dword t >> 1): half
// the LDS, twice the resident workgroups.  Counters and offsets stay below 65536 because n_items does.
template <bool U16>
struct Hist {
    uint32_t *h;
    __device__ __forceinline__ uint32_t *slot(int bin, int t) const
    {
        return U16 ? h + bin * (kTopkThreads / 2) + (t >> 1) : h + bin * kTopkThreads + t;
    }
    __device__ __forceinline__ void add(int bin, int t) const
    {
        __hip_atomic_fetch_add(slot(bin, t), U16 ? (1u << (16 * (t & 1))) : 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ uint32_t fetch_inc(int bin, int t) const
    {
        const uint32_t old = __hip_atomic_fetch_add(slot(bin, t), U16 ? (1u << (16 * (t & 1))) : 1u,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return U16 ? (old >> (16 * (t & 1))) & 0xffffu : old;
    }
    // the four counters of threads 4*lane .. 4*lane+3 of one bin
    __device__ __forceinline__ uint4 load4(int bin, int lane) const
    {
        if (U16) {
            const uint2 v = *reinterpret_cast<const uint2 *>(h + bin * (kTopkThreads / 2) + 2 * lane);
            return make_uint4(v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16);
        }
        return *reinterpret_cast<const uint4 *>(h + bin * kTopkThreads + 4 * lane);
    }
    __device__ __forceinline__ void store4(int bin, int lane, uint4 o) const
    {
        if (U16)
            *reinterpret_cast<uint2 *>(h + bin * (kTopkThreads / 2) + 2 * lane) = make_uint2(o.x | (o.y << 16), o.z | (o.w << 16));
        else
            *reinterpret_cast<uint4 *>(h + bin * kTopkThreads + 4 * lane) = o;
    }
    static __host__ __device__ size_t words(int nbins) { return (size_t)nbins * (U16 ? kTopkThreads / 2 : kTopkThreads); }
};

// The ranked indices leave with k scattered 4-byte global stores per query.  Placing them in an LDS row first and copying
// it out with 16-byte coalesced stores was measured on MI355X (c1 shape): it costs a resident workgroup per CU (53 KB vs
// 34 KB of LDS) and ran 163 us vs 117 us -- the kernel is latency-bound, so occupancy wins -- and was removed.
template <typename Source, bool U16>
__device__ __forceinline__ void rank_one_query(const Source &src, int64_t n_items, int C, int nbins,
                                               int k, int32_t *__restrict__ idx_out,
                                               uint8_t *__restrict__ dist_out, uint32_t *lds,
                                               uint32_t *__restrict__ cum_out = nullptr)
{
    Hist<U16> hist{lds};
    uint32_t *tot = lds + Hist<U16>::words(nbins);     // kMaxBins
    uint32_t *base = tot + kMaxBins;                   // kMaxBins + 1
    uint32_t *misc = base + kMaxBins + 1;              // [0] = threshold bin T
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();

    {   // zero the table with 16-byte stores
        uint4 *h4 = reinterpret_cast<uint4 *>(lds);
        const int n4 = (int)(Hist<U16>::words(nbins) / 4);
        for (int i = tid; i < n4; i += kTopkThreads) h4[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    // ---- phase 1: private-column histogram.  A column belongs to one thread, so the LDS adds never
    // contend; nothing waits on them.  Distances of the next UNR items are computed while they drain.
    const int64_t first = (int64_t)tid * C;
    // items of this thread that exist (only the last threads of the last column are short)
    const int nvalid = (int)min((int64_t)C, max((int64_t)0, n_items - first));
    constexpr int UNR = 16;
    using Raw = typename Source::Raw;
    const int nfull = C / UNR;
    // Columns of at most kCacheItems items keep their distances (one byte each) in registers between the
    // two phases, so phase 2 neither reloads the codes nor recomputes the popcounts.
    constexpr int kCacheItems = 128, kCacheBatches = kCacheItems / UNR;
    const bool cached = C <= kCacheItems;            // uniform
    uint32_t dcache[kCacheItems / 4];
    if (cached) {
#pragma unroll
        for (int bi = 0; bi < kCacheBatches; ++bi) {
            if (bi * UNR < C) {                       // uniform
                Raw cur[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) cur[u] = src.fetch(min(bi * UNR + u, C - 1), tid, first + bi * UNR + u);
#pragma unroll
                for (int u4 = 0; u4 < UNR / 4; ++u4) {
                    uint32_t word = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int u = 4 * u4 + j;
                        const int d = src.dist(cur[u]);
                        word |= (uint32_t)d << (8 * j);
                        if (bi * UNR + u < nvalid) hist.add(d, tid);
                    }
                    dcache[bi * (UNR / 4) + u4] = word;
                }
            }
        }
    } else {
        Raw cur[UNR], nxt[UNR];
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) cur[u] = src.fetch(u, tid, first + u);
        }
        for (int bi = 0; bi < nfull; ++bi) {
            const int r = bi * UNR;
            if (bi + 1 < nfull) {   // the next batch's loads are in flight while this one is counted
#pragma unroll
                for (int u = 0; u < UNR; ++u) nxt[u] = src.fetch(r + UNR + u, tid, first + r + UNR + u);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                if (r + u < nvalid) hist.add(src.dist(cur[u]), tid);
#pragma unroll
            for (int u = 0; u < UNR; ++u) cur[u] = nxt[u];
        }
        for (int r = nfull * UNR; r < nvalid; ++r) hist.add(src.dist(src.fetch(r, tid, first + r)), tid);
    }
    __syncthreads();

    // ---- per-bin totals (wave w takes bins w, w+4, ...)
    for (int b = wv; b < nbins; b += kTopkThreads / 64) {
        const uint4 v = hist.load4(b, lane);
        const uint32_t s = wave_sum_u32(v.x + v.y + v.z + v.w);
        if (lane == 0) tot[b] = s;
    }
    __syncthreads();

    // ---- exclusive scan over bins (wave 0; up to 3 bins per lane covers 192 >= 130 bins)
    if (wv == 0) {
        const int b0 = 3 * lane;
        const uint32_t t[3] = {b0 < nbins ? tot[b0] : 0u, b0 + 1 < nbins ? tot[b0 + 1] : 0u, b0 + 2 < nbins ? tot[b0 + 2] : 0u};
        const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
        const uint32_t excl = bin_scan3(t, nbins, base, lane), incl = excl + t0 + t1 + t2;
        if (lane == 63) base[nbins] = incl;  // = n_items
        // threshold bin: first bin whose inclusive count reaches k
        int cand = nbins;  // sentinel
        if (b0 < nbins && excl + t0 >= (uint32_t)k) cand = b0;
        else if (b0 + 1 < nbins && excl + t0 + t1 >= (uint32_t)k) cand = b0 + 1;
        else if (b0 + 2 < nbins && excl + t0 + t1 + t2 >= (uint32_t)k) cand = b0 + 2;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cand = min(cand, __shfl_xor(cand, d, 64));
        if (lane == 0) misc[0] = (uint32_t)min(cand, nbins - 1);
    }
    __syncthreads();
    const int T = (int)misc[0];
    // cumulative histogram of ALL items (cum[b] = #items with distance < b): lets a sharded search derive the
    // global threshold from one small all-reduce instead of exchanging full-length lists
    if (cum_out)
        for (int b = tid; b <= nbins; b += kTopkThreads) cum_out[b] = base[b];

    // ---- per-bin exclusive scan over threads, plus the bin base -> starting output offsets
    for (int b = wv; b <= T; b += kTopkThreads / 64) {
        const uint4 v = hist.load4(b, lane);
        const uint32_t s = v.x + v.y + v.z + v.w;
        const uint32_t excl = wave_incl_scan_u32(s) - s + base[b];
        uint4 o;
        o.x = excl;
        o.y = excl + v.x;
        o.z = o.y + v.y;
        o.w = o.z + v.z;
        hist.store4(b, lane, o);
    }
    __syncthreads();

    // ---- phase 2: stable placement of the items in bins <= T (returning LDS adds, UNR in flight)
    // `store` is always true (every caller has checked k >= 1 on the host), and uniform.  ANDed into the store conditions it keeps each batch's sixteen stores one chain of
    // skip-branches; without it the compiler duplicates the chain into a taken and a skipped copy (measured: c3 shard + 1 %),
    // and with a likely-hint in its place shards ranked at k = N ran 10 % slower.
    const bool store = k > 0;
    if (cached) {
#pragma unroll
        for (int bi = 0; bi < kCacheBatches; ++bi) {
            if (bi * UNR < C) {
                uint32_t pos[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int d = (dcache[bi * (UNR / 4) + u / 4] >> (8 * (u & 3))) & 0xff;
                    pos[u] = 0xffffffffu;
                    if (bi * UNR + u < nvalid && d <= T) pos[u] = hist.fetch_inc(d, tid);
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u)
                    if (pos[u] < (uint32_t)k && store) idx_out[pos[u]] = src.id(first + bi * UNR + u);
            }
        }
    } else {
        Raw cur[UNR], nxt[UNR];
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) cur[u] = src.fetch(u, tid, first + u);
        }
        for (int bi = 0; bi < nfull; ++bi) {
            const int r = bi * UNR;
            if (bi + 1 < nfull) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) nxt[u] = src.fetch(r + UNR + u, tid, first + r + UNR + u);
            }
            uint32_t pos[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int d = src.dist(cur[u]);
                pos[u] = 0xffffffffu;
                if (r + u < nvalid && d <= T) pos[u] = hist.fetch_inc(d, tid);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                if (pos[u] < (uint32_t)k && store) idx_out[pos[u]] = src.id(first + r + u);
#pragma unroll
            for (int u = 0; u < UNR; ++u) cur[u] = nxt[u];
        }
        for (int r = nfull * UNR; r < nvalid; ++r) {
            const int64_t item = first + r;
            const int d = src.dist(src.fetch(r, tid, item));
            if (d <= T) {
                const uint32_t pos = hist.fetch_inc(d, tid);
                if (pos < (uint32_t)k && store) idx_out[pos] = src.id(item);
            }
        }
    }

    // ---- distance row from the bin boundaries: dist[p] = b  with  base[b] <= p < base[b+1].
    // Each thread owns a run of positions: one binary search, then it walks the boundaries; 4 bytes per store.
    if (dist_out) {
        const int chunk = ((k + kTopkThreads - 1) / kTopkThreads + 3) & ~3;
        const int p0 = tid * chunk;
        if (p0 < k) {
            int lo = 0, hi = nbins;  // invariant: base[lo] <= p0 < base[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (base[mid] <= (uint32_t)p0) lo = mid;
                else hi = mid;
            }
            int bin = lo;
            uint32_t next = base[bin + 1];
            const bool aligned = (reinterpret_cast<uintptr_t>(dist_out) & 3) == 0;
            for (int i = 0; i < chunk; i += 4) {
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t p = (uint32_t)(p0 + i + j);
                    while (p >= next && bin + 1 < nbins) { ++bin; next = base[bin + 1]; }
                    word |= (uint32_t)bin << (8 * j);
                }
                if (aligned && p0 + i + 4 <= k) {
                    *reinterpret_cast<uint32_t *>(dist_out + p0 + i) = word;
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (p0 + i + j < k) dist_out[p0 + i + j] = (uint8_t)(word >> (8 * j));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------ kernels
template <int WORDS>
__global__ __launch_bounds__(kTopkThreads) void k_transpose_db(const uint64_t *__restrict__ db,
                                                               uint64_t *__restrict__ dbT,
                                                               int64_t N, int C)
{
    const int64_t total = (int64_t)C * kTopkThreads;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / kTopkThreads;
        const int t = (int)(i - r * kTopkThreads);
        const int64_t item = (int64_t)t * C + r;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) dbT[i * WORDS + w] = item < N ? db[item * WORDS + w] : 0ull;
    }
}

template <int WORDS, bool U16>
__global__ __launch_bounds__(kTopkThreads) void k_hamming_topk(const uint64_t *__restrict__ q,
                                                               const uint64_t *__restrict__ dbT,
                                                               int32_t *__restrict__ idx,
                                                               uint8_t *__restrict__ dist, int64_t N,
                                                               int C, int nbins, int k,
                                                               int64_t idx_offset, uint32_t *__restrict__ cum)
{
    extern __shared__ uint4 lds4[];
    const int qi = blockIdx.x;
    CodeSource<WORDS> src;
    src.dbT = dbT;
    src.idx_offset = idx_offset;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) src.qw[w] = q[(int64_t)qi * WORDS + w];
    rank_one_query<CodeSource<WORDS>, U16>(src, N, C, nbins, k, idx + (int64_t)qi * k,
                                           dist ? dist + (int64_t)qi * k : nullptr, reinterpret_cast<uint32_t *>(lds4),
                                           cum ? cum + (int64_t)qi * (nbins + 1) : nullptr);
}

template <bool U16>
__global__ __launch_bounds__(kTopkThreads) void k_rank_from_dist(const uint8_t *__restrict__ dmat,
                                                                 int64_t ld, int64_t N,
                                                                 int32_t *__restrict__ idx,
                                                                 uint8_t *__restrict__ dist, int k,
                                                                 int C, int nbins)
{
    extern __shared__ uint4 lds4[];
    const int qi = blockIdx.x;
    RowSource src;
    src.row = dmat + (int64_t)qi * ld;
    src.n = N;
    rank_one_query<RowSource, U16>(src, N, C, nbins, k, idx + (int64_t)qi * k, dist ? dist + (int64_t)qi * k : nullptr,
                                   reinterpret_cast<uint32_t *>(lds4));
}

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
    int32_t *start = reinterpret_cast<int32_t *>(lds4);           // [G][nbins + 1]: first position with dist >= b
    int32_t *delta = start + G * (nbins + 1);                     // [G][nbins]
    uint32_t *base = reinterpret_cast<uint32_t *>(delta + G * nbins);   // [nbins + 1]
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

// ------------------------------------------------------------------------ average precision
// AP over a ranked list (accuracy_calculator.py:222-229): hits at 1-based ranks r_1 < r_2 < ...
// give AP = mean_j (j / r_j); relevance = labels share a bit (label_comparison_fn :31-37).
template <int LW>
__global__ __launch_bounds__(256) void k_map_at_k(const int32_t *__restrict__ idx, int64_t ld, int k,
                                                  const uint64_t *__restrict__ qlab,
                                                  const uint64_t *__restrict__ dblab, int lwords,
                                                  float *__restrict__ ap, int32_t *__restrict__ nrel)
{
    __shared__ uint32_t wave_cnt[4];
    __shared__ double wave_sum[4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int32_t *list = idx + (int64_t)qi * ld;
    const int lw = LW > 0 ? LW : lwords;
    uint64_t ql[LW > 0 ? LW : 1];
    if constexpr (LW > 0) {
#pragma unroll
        for (int w = 0; w < LW; ++w) ql[w] = qlab[(int64_t)qi * LW + w];
    }
    uint32_t running = 0;
    double acc = 0.0;
    for (int p0 = 0; p0 < k; p0 += 256) {
        const int p = p0 + tid;
        bool rel = false;
        if (p < k) {
            const int32_t id = list[p];
            if (id >= 0) {
                const uint64_t *dl = dblab + (int64_t)id * lw;
                if constexpr (LW > 0) {
                    uint64_t any = 0;
#pragma unroll
                    for (int w = 0; w < LW; ++w) any |= dl[w] & ql[w];
                    rel = any != 0;
                } else {
                    uint64_t any = 0;
                    for (int w = 0; w < lw; ++w) any |= dl[w] & qlab[(int64_t)qi * lw + w];
                    rel = any != 0;
                }
            }
        }
        const uint64_t mask = __ballot(rel);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = running;
        for (int w2 = 0; w2 < wv; ++w2) before += wave_cnt[w2];
        const uint32_t block_total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (rel) {
            const uint32_t j = before + (uint32_t)mbcnt(mask) + 1;  // this is the j-th hit
            acc += (double)((float)j / (float)(p + 1));             // fp32 quotient like the reference
        }
        running += block_total;
        __syncthreads();
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) wave_sum[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        const double s = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        ap[qi] = running ? (float)(s / (double)running) : 0.0f;
        if (nrel) nrel[qi] = (int32_t)running;
    }
}

// Running hit count along a ranked list: hits[q][p] = number of relevant entries among list[0..p]
// (relevance as in k_map_at_k).  Precision@p, recall@p, R-precision and the precision/recall curves of
// accuracy_calculator.py:131-181,235-273 are ratios of these counts.
__global__ __launch_bounds__(256) void k_hit_prefix(const int32_t *__restrict__ idx, int k,
                                                    const uint64_t *__restrict__ qlab,
                                                    const uint64_t *__restrict__ dblab, int lwords,
                                                    uint32_t *__restrict__ hits)
{
    __shared__ uint32_t wave_cnt[4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int32_t *list = idx + (int64_t)qi * k;
    uint32_t running = 0;
    for (int p0 = 0; p0 < k; p0 += 256) {
        const int p = p0 + tid;
        bool rel = false;
        if (p < k) {
            const int32_t id = list[p];
            if (id >= 0) {
                uint64_t any = 0;
                for (int w = 0; w < lwords; ++w) any |= dblab[(int64_t)id * lwords + w] & qlab[(int64_t)qi * lwords + w];
                rel = any != 0;
            }
        }
        const uint64_t mask = __ballot(rel);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = running;
        for (int w2 = 0; w2 < wv; ++w2) before += wave_cnt[w2];
        if (p < k) hits[(int64_t)qi * k + p] = before + (uint32_t)mbcnt(mask) + (rel ? 1u : 0u);
        running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
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
    int32_t *start = reinterpret_cast<int32_t *>(lds4);           // [G][nbins + 1]: first position with dist >= b
    int32_t *delta = start + G * (nbins + 1);                     // [G][nbins]
    uint32_t *base = reinterpret_cast<uint32_t *>(delta + G * nbins);   // [nbins + 1]
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

template <int WORDS>
static int launch_transpose(const uint64_t *db, uint64_t *dbT, int64_t N, hipStream_t st)
{
    const int C = (int)ceil_div(N, kTopkThreads);
    const int64_t total = (int64_t)C * kTopkThreads;
    hipLaunchKernelGGL((k_transpose_db<WORDS>), dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 4096)),
                       dim3(256), 0, st, db, dbT, N, C);
    WV_CHECK_LAUNCH("k_transpose_db");
    return WV_OK;
}

// The image the plan's kernel reads: inside the prepared blob, or built into the workspace first (one extra small launch
// per call).
static int rank_image(const RankPlan &plan, const uint64_t *db, const void *prepared, void *ws, int64_t N, int words,
                      hipStream_t st, const void **img)
{
    if (prepared) {
        *img = blob_image(prepared, N, words, plan.kernel);
        return WV_OK;
    }
    *img = ws;
    if (plan.kernel != RankKernel::column) return rank2_prepare(db, ws, N, words, plan.kernel, st);
    return words == 1 ? launch_transpose<1>(db, (uint64_t *)ws, N, st) : launch_transpose<2>(db, (uint64_t *)ws, N, st);
}

template <int WORDS>
static int launch_column(const RankPlan &plan, const uint64_t *q, const void *img, int32_t *idx, uint8_t *dist, int Q, int64_t N,
                         int nbits, int k, int64_t idx_offset, uint32_t *cum, hipStream_t st)
{
    auto kern = column_u16(N) ? k_hamming_topk<WORDS, true> : k_hamming_topk<WORDS, false>;
    int rc = set_lds_attr(reinterpret_cast<const void *>(kern), plan.lds, "hamming_topk");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(Q), dim3(kTopkThreads), plan.lds, st, q, (const uint64_t *)img, idx, dist, N, plan.C, nbits + 1, k,
                       idx_offset, cum);
    WV_CHECK_LAUNCH("k_hamming_topk");
    return WV_OK;
}

// int32 lists (+ distance rows, + histograms) from the codes: wv_hamming_topk / _prepared / _ex
static int launch_topk(const uint64_t *q, const uint64_t *db, const void *prepared, int32_t *idx, uint8_t *dist, int Q, int64_t N,
                       int nbits, int k, int64_t idx_offset, void *ws, hipStream_t st, uint32_t *cum = nullptr)
{
    const RankPlan plan = rank_plan(Q, N, nbits, k, RankMode::lists);
    const void *img = nullptr;
    int rc = rank_image(plan, db, prepared, ws, N, (nbits + 63) / 64, st, &img);
    if (rc) return rc;
    if (plan.kernel != RankKernel::column) return rank2_launch(plan, q, img, idx, nullptr, dist, cum, Q, N, nbits, k, idx_offset, st);
    if (nbits <= 64) return launch_column<1>(plan, q, img, idx, dist, Q, N, nbits, k, idx_offset, cum, st);
    return launch_column<2>(plan, q, img, idx, dist, Q, N, nbits, k, idx_offset, cum, st);
}

static int require_nbits(const char *what, int nbits)
{
    WV_REQUIRE(nbits >= 1 && nbits <= 128, "%s: nbits=%d (supported: 1..128)", what, nbits);
    return WV_OK;
}

// The argument checks the ranking entry points share: buffers, shape and code width (all a call without k needs) ...
static int validate_rank_shape(const char *what, bool buffers, int Q, int64_t N, int nbits)
{
    WV_REQUIRE(buffers, "%s: null buffer", what);
    WV_REQUIRE(Q >= 0 && N >= 1, "%s: bad shape Q=%d N=%lld", what, Q, (long long)N);
    return require_nbits(what, nbits);
}

// ... and the list length
static int validate_rank_args(const char *what, bool buffers, int Q, int64_t N, int nbits, int k)
{
    if (int rc = validate_rank_shape(what, buffers, Q, N, nbits)) return rc;
    WV_REQUIRE(k >= 1 && k <= N, "%s: k=%d must be in [1, N=%lld] (torch.topk raises too)", what, k, (long long)N);
    return WV_OK;
}

// ... and of those that return global row numbers as int32
static int validate_rank_ids(const char *what, bool buffers, int Q, int64_t N, int nbits, int k, int64_t idx_offset)
{
    if (int rc = validate_rank_args(what, buffers, Q, N, nbits, k)) return rc;
    WV_REQUIRE(N + idx_offset <= 0x7fffffffLL && idx_offset >= 0, "%s: indices exceed int32", what);
    return WV_OK;
}

// Prepared blobs and workspaces hold the kernels' images, which are read and written 16 bytes at a time (uint4): a caller that
// carves one out of a larger arena at another alignment is refused here, before anything is launched (NULL passes: absent).
static int require_aligned16(const char *what, const char *name, const void *p)
{
    WV_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, "%s: %s must be 16-byte aligned", what, name);
    return WV_OK;
}

static int require_workspace(const char *what, const void *workspace, size_t workspace_bytes, int Q, int64_t N, int nbits, int k)
{
    const size_t need = wv_hamming_topk_workspace_bytes(Q, N, (nbits + 63) / 64, k);
    if (!workspace || workspace_bytes < need) WV_FAIL(WV_ENOMEM, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return require_aligned16(what, "workspace", workspace);
}

}  // namespace wv

using namespace wv;

extern "C" size_t wv_hamming_topk_workspace_bytes(int Q, int64_t N, int words, int k)
{
    (void)Q; (void)k;                                            // ABI: sized without knowing the call, so for any plan's image
    if (N <= 0 || words <= 0) return 0;
    return std::max({rank_image_bytes(RankKernel::column, N, words), rank_image_bytes(RankKernel::window256, N, words),
                     rank_image_bytes(RankKernel::window64, N, words)});
}

extern "C" int wv_hamming_topk(const uint64_t *q, const uint64_t *db, int32_t *idx, uint8_t *dist,
                               int Q, int64_t N, int nbits, int k, int64_t idx_offset,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_ids("hamming_topk", q && db && idx, Q, N, nbits, k, idx_offset)) return rc;
    if (int rc = require_workspace("hamming_topk", workspace, workspace_bytes, Q, N, nbits, k)) return rc;
    if (Q == 0) return WV_OK;
    return launch_topk(q, db, nullptr, idx, dist, Q, N, nbits, k, idx_offset, workspace, (hipStream_t)stream);
}

extern "C" size_t wv_db_prepared_bytes(int64_t N, int words)
{
    if (N <= 0 || words < 1 || words > 4) return 0;
    return blob_layout(N, words).total;
}

extern "C" int wv_db_prepare(const uint64_t *db, int64_t N, int words, void *prepared, size_t prepared_bytes,
                             void *stream)
{
    WV_REQUIRE(db && prepared, "db_prepare: null buffer");
    WV_REQUIRE(N >= 1 && words >= 1 && words <= 4, "db_prepare: bad shape N=%lld words=%d", (long long)N, words);
    if (int rc = require_aligned16("db_prepare", "prepared", prepared)) return rc;
    const BlobLayout L = blob_layout(N, words);
    if (prepared_bytes < L.total) WV_FAIL(WV_ENOMEM, "db_prepare: buffer %zu < %zu bytes", prepared_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char *blob = (char *)prepared;
    int rc = dist_prepare(db, prepared, N, words, st);
    if (rc || words > 2) return rc;                              // the ranking images exist for codes of <= 2 words
    rc = words == 1 ? launch_transpose<1>(db, (uint64_t *)(blob + L.column), N, st) : launch_transpose<2>(db, (uint64_t *)(blob + L.column), N, st);
    if (!rc && N <= kImg256MaxRows) rc = rank2_prepare(db, blob + L.window256, N, words, RankKernel::window256, st);
    if (!rc && N <= kImg64MaxRows) rc = rank2_prepare(db, blob + L.window64, N, words, RankKernel::window64, st);
    return rc;
}

extern "C" int wv_hamming_topk_prepared(const uint64_t *q, const void *prepared, int32_t *idx, uint8_t *dist, int Q,
                                        int64_t N, int nbits, int k, int64_t idx_offset, void *stream)
{
    if (int rc = validate_rank_ids("hamming_topk_prepared", q && prepared && idx, Q, N, nbits, k, idx_offset)) return rc;
    if (int rc = require_aligned16("hamming_topk_prepared", "prepared", prepared)) return rc;
    if (Q == 0) return WV_OK;
    return launch_topk(q, nullptr, prepared, idx, dist, Q, N, nbits, k, idx_offset, nullptr, (hipStream_t)stream);
}

extern "C" int wv_topk_merge(const int32_t *idx_in, const uint8_t *dist_in, int G, int Q, int kin,
                             int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream)
{
    WV_REQUIRE(idx_in && dist_in && idx_out, "topk_merge: null buffer");
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1, "topk_merge: bad shape G=%d Q=%d kin=%d", G, Q, kin);
    if (int rc = require_nbits("topk_merge", nbits)) return rc;
    WV_REQUIRE(k >= 1 && (int64_t)k <= (int64_t)G * kin, "topk_merge: k=%d > G*kin", k);
    if (Q == 0) return WV_OK;
    const int nbins = nbits + 2;  // dist = nbits + 1 marks padding entries: they rank after every real one
    const size_t lds = ((size_t)G * (nbins + 1) + (size_t)G * nbins + nbins + 1 + 4) * 4;
    WV_REQUIRE(lds <= 60 * 1024, "topk_merge: too many shards (G=%d)", G);
    hipLaunchKernelGGL(k_merge_sorted, dim3(Q), dim3(256), lds, (hipStream_t)stream, idx_in, dist_in, G, Q, kin,
                       idx_out, dist_out, k, nbins);
    WV_CHECK_LAUNCH("k_merge_sorted");
    return WV_OK;
}

namespace wv {
// Sharded mAP, receiving side: per query the G shards' relevance strings (bit p = is the shard's p-th nearest row relevant)
// and cumulative histograms -> average precision.  The global list orders entries by (distance, shard, position), so the
// merged relevance string is the concatenation, bin by bin and shard by shard, of runs of the shards' strings; it is
// assembled in LDS (k bits) with shifted 32-bit copies and walked exactly as k_map_at_k walks a list (ap_walk.hpp).
// need_out: as in k_merge_cum.
// Assembles the merged string of query blockIdx.x in LDS (layout above); ends with a workgroup barrier.  M: the string,
// scratch: free LDS behind it (8-byte aligned).
__device__ __forceinline__ void merge_relbits_string(uint4 *lds4, const uint32_t *__restrict__ relbits, const uint32_t *__restrict__ cum,
                                                     int G, int Q, int kin, int w32, int k, int nbins, int32_t *__restrict__ need_out,
                                                     int64_t rb_ld32, int64_t cum_ld, uint32_t *&M, uint32_t *&scratch)
{
    int32_t *start = reinterpret_cast<int32_t *>(lds4);           // [G][nbins + 1]: first position with dist >= b
    uint32_t *base = reinterpret_cast<uint32_t *>(start + G * (nbins + 1));   // [nbins + 1]
    M = base + nbins + 1;                                         // merged relevance string, k bits (+ spill word)
    const int mwords = (k + 31) / 32 + 1;
    scratch = M + mwords + (mwords & 1);                          // ap_final's doubles: 8-byte aligned
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

__global__ __launch_bounds__(256) void k_merge_relbits_ap(const uint32_t *__restrict__ relbits, const uint32_t *__restrict__ cum,
                                                          int G, int Q, int kin, int w32, int k, int nbins,
                                                          float *__restrict__ ap, int32_t *__restrict__ nrel,
                                                          int32_t *__restrict__ need_out, int64_t rb_ld32, int64_t cum_ld)
{
    extern __shared__ uint4 lds4[];
    uint32_t *M, *scratch;
    merge_relbits_string(lds4, relbits, cum, G, Q, kin, w32, k, nbins, need_out, rb_ld32, cum_ld, M, scratch);
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

// One chunk of relevance bits -> the walk at several cut-offs: what the merge and the list kernel below share.  rel_at(p) =
// relevance of list position p < k (free of side effects: the last position is asked again for the padding of the last
// round); ap / nrel: the query's rows of cuts.n entries.
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
    for (int c0 = 0; c0 < R; c0 += kApRounds) {
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

// k_merge_relbits_ap at several cut-offs: the string is assembled for k = the largest, ap / nrel are [Q][cuts.n].
__global__ __launch_bounds__(256) void k_merge_relbits_ap_cuts(const uint32_t *__restrict__ relbits, const uint32_t *__restrict__ cum,
                                                               int G, int Q, int kin, int w32, int nbins, float *__restrict__ ap,
                                                               int32_t *__restrict__ nrel, int32_t *__restrict__ need_out,
                                                               int64_t rb_ld32, int64_t cum_ld, ApCuts cuts)
{
    extern __shared__ uint4 lds4[];
    const int k = cuts.k[cuts.n - 1], qi = blockIdx.x;
    uint32_t *M, *scratch;
    merge_relbits_string(lds4, relbits, cum, G, Q, kin, w32, k, nbins, need_out, rb_ld32, cum_ld, M, scratch);
    walk_cuts_256([M](int p) { return ((M[p >> 5] >> (p & 31)) & 1u) != 0; }, k, scratch, cuts, ap + (int64_t)qi * cuts.n,
                  nrel ? nrel + (int64_t)qi * cuts.n : nullptr);
}

// k_map_at_k at several cut-offs: the list is read and the labels are gathered once, ap / nrel are [Q][cuts.n].  The walk is
// ap_walk.hpp's, whose order is k_map_at_k's: every column has the bits of a k_map_at_k launch with that k.
template <int LW>
__global__ __launch_bounds__(256) void k_map_at_ks(const int32_t *__restrict__ idx, int64_t ld, const uint64_t *__restrict__ qlab,
                                                   const uint64_t *__restrict__ dblab, int lwords, float *__restrict__ ap,
                                                   int32_t *__restrict__ nrel, ApCuts cuts)
{
    __shared__ __attribute__((aligned(8))) uint32_t scratch[ap_cuts_scratch_dwords<256>()];
    const int qi = blockIdx.x, k = cuts.k[cuts.n - 1];
    const int32_t *list = idx + (int64_t)qi * ld;
    const int lw = LW > 0 ? LW : lwords;
    const uint64_t *ql = qlab + (int64_t)qi * lw;
    uint64_t qreg[LW > 0 ? LW : 1];
    if constexpr (LW > 0) {
#pragma unroll
        for (int w = 0; w < LW; ++w) qreg[w] = ql[w];
    }
    auto rel_at = [&](int p) {
        const int32_t id = list[p];
        const uint64_t *dl = dblab + (int64_t)max(id, 0) * lw;   // an absent entry (< 0) reads row 0 and counts as no hit
        uint64_t any = 0;
        if constexpr (LW > 0) {
#pragma unroll
            for (int w = 0; w < LW; ++w) any |= dl[w] & qreg[w];
        } else {
            for (int w = 0; w < lw; ++w) any |= dl[w] & ql[w];
        }
        return id >= 0 && any != 0;
    };
    walk_cuts_256(rel_at, k, scratch, cuts, ap + (int64_t)qi * cuts.n, nrel ? nrel + (int64_t)qi * cuts.n : nullptr);
}
}  // namespace wv

extern "C" int wv_topk_merge_cum_need(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin, int64_t shard_rows,
                                      int32_t *idx_out, uint8_t *dist_out, int k, int nbits, int32_t *need_out, void *stream);

extern "C" int wv_topk_merge_cum(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin,
                                 int64_t shard_rows, int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream)
{
    return wv_topk_merge_cum_need(idx_local, cum, G, Q, kin, shard_rows, idx_out, dist_out, k, nbits, nullptr, stream);
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
    const size_t lds = ((size_t)G * (nbins + 1) + (size_t)G * nbins + nbins + 1 + 4) * 4;
    WV_REQUIRE(lds <= 60 * 1024, "topk_merge_cum: too many shards (G=%d)", G);
    hipLaunchKernelGGL(k_merge_cum, dim3(Q), dim3(256), lds, (hipStream_t)stream, idx_local, cum, G, Q, kin, shard_rows,
                       idx_out, dist_out, k, nbins, need_out);
    WV_CHECK_LAUNCH("k_merge_cum");
    return WV_OK;
}

extern "C" int wv_rank_from_dist(const uint8_t *dist_matrix, int64_t ld_dist, int Q, int64_t N,
                                 int nbits, int32_t *idx, uint8_t *dist, int k, void *stream)
{
    if (int rc = validate_rank_ids("rank_from_dist", dist_matrix && idx, Q, N, nbits, k, 0)) return rc;
    WV_REQUIRE(ld_dist >= N, "rank_from_dist: row pitch %lld < N=%lld", (long long)ld_dist, (long long)N);
    if (Q == 0) return WV_OK;
    const RankPlan plan = rank_plan_column(N, nbits);            // stored distance rows: the column kernel is the only taker
    auto kern = column_u16(N) ? k_rank_from_dist<true> : k_rank_from_dist<false>;
    if (int rc = set_lds_attr(reinterpret_cast<const void *>(kern), plan.lds, "rank_from_dist")) return rc;
    hipLaunchKernelGGL(kern, dim3(Q), dim3(kTopkThreads), plan.lds, (hipStream_t)stream, dist_matrix, ld_dist, N, idx, dist, k,
                       plan.C, nbits + 1);
    WV_CHECK_LAUNCH("k_rank_from_dist");
    return WV_OK;
}

extern "C" int wv_map_at_k_ld(const int32_t *idx, int64_t ld, int Q, int k, const uint64_t *qlab,
                              const uint64_t *dblab, int lwords, float *ap, int32_t *nrel, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && ap, "map_at_k: null buffer");
    WV_REQUIRE(Q >= 0 && k >= 1 && lwords >= 1 && ld >= k, "map_at_k: bad shape Q=%d k=%d ld=%lld lwords=%d", Q, k, (long long)ld, lwords);
    if (Q == 0) return WV_OK;
    hipStream_t st = (hipStream_t)stream;
    if (lwords == 1)
        hipLaunchKernelGGL((k_map_at_k<1>), dim3(Q), dim3(256), 0, st, idx, ld, k, qlab, dblab, lwords, ap, nrel);
    else if (lwords == 2)
        hipLaunchKernelGGL((k_map_at_k<2>), dim3(Q), dim3(256), 0, st, idx, ld, k, qlab, dblab, lwords, ap, nrel);
    else
        hipLaunchKernelGGL((k_map_at_k<0>), dim3(Q), dim3(256), 0, st, idx, ld, k, qlab, dblab, lwords, ap, nrel);
    WV_CHECK_LAUNCH("k_map_at_k");
    return WV_OK;
}

extern "C" int wv_map_at_k(const int32_t *idx, int Q, int k, const uint64_t *qlab,
                           const uint64_t *dblab, int lwords, float *ap, int32_t *nrel, void *stream)
{
    return wv_map_at_k_ld(idx, k, Q, k, qlab, dblab, lwords, ap, nrel, stream);
}

extern "C" int wv_hit_prefix(const int32_t *idx, int Q, int k, const uint64_t *qlab, const uint64_t *dblab,
                             int lwords, uint32_t *hits, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && hits, "hit_prefix: null buffer");
    WV_REQUIRE(Q >= 0 && k >= 1 && lwords >= 1, "hit_prefix: bad shape Q=%d k=%d lwords=%d", Q, k, lwords);
    if (Q == 0) return WV_OK;
    hipLaunchKernelGGL(k_hit_prefix, dim3(Q), dim3(256), 0, (hipStream_t)stream, idx, k, qlab, dblab, lwords, hits);
    WV_CHECK_LAUNCH("k_hit_prefix");
    return WV_OK;
}

extern "C" int wv_hamming_topk_ex(const uint64_t *q, const uint64_t *db, const void *prepared, int32_t *idx,
                                  uint8_t *dist, uint32_t *cum, int Q, int64_t N, int nbits, int k, int64_t idx_offset,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_ids("hamming_topk_ex", q && idx && (db || prepared), Q, N, nbits, k, idx_offset)) return rc;
    if (int rc = require_aligned16("hamming_topk_ex", "prepared", prepared)) return rc;
    if (Q == 0) return WV_OK;
    if (!prepared)
        if (int rc = require_workspace("hamming_topk_ex", workspace, workspace_bytes, Q, N, nbits, k)) return rc;
    return launch_topk(q, db, prepared, idx, dist, Q, N, nbits, k, idx_offset, workspace, (hipStream_t)stream, cum);
}

// ---------------------------------------------------------------------------------- mAP without the lists
extern "C" size_t wv_rank_labels_prepared_bytes(int64_t N, int lwords)
{
    if (N < 1 || N > kImg256MaxRows || lwords < 1 || lwords > 2) return 0;
    return rank2_labels_bytes(N, lwords);
}

extern "C" int wv_rank_labels_prepare(const uint64_t *dblab, int64_t N, int lwords, void *prepared_labels, size_t prepared_bytes,
                                      void *stream)
{
    WV_REQUIRE(dblab && prepared_labels, "rank_labels_prepare: null buffer");
    const size_t need = wv_rank_labels_prepared_bytes(N, lwords);
    if (!need)
        WV_FAIL(WV_ENOTSUP, "rank_labels_prepare: %lld rows x %d label words are outside the fused kernels (<= 32768 rows, <= 128 classes)",
                (long long)N, lwords);
    if (prepared_bytes < need) WV_FAIL(WV_ENOMEM, "rank_labels_prepare: buffer %zu < %zu bytes", prepared_bytes, need);
    if (int rc = require_aligned16("rank_labels_prepare", "prepared_labels", prepared_labels)) return rc;
    return rank2_labels_prepare(dblab, prepared_labels, N, lwords, (hipStream_t)stream);
}

// ranking + AP / relevance strings (RankMode::ap, relbits): windowed kernel on the prepared images, or WV_ENOTSUP
static int fused_call(const char *what, RankMode mode, const uint64_t *q, const void *prepared, const Rank2Ap &apx, uint32_t *cum, int Q,
                      int64_t N, int nbits, int k, void *stream)
{
    if (int rc = require_aligned16(what, "prepared", prepared)) return rc;
    if (int rc = require_aligned16(what, "prepared_labels", apx.cls)) return rc;
    const RankPlan plan = rank_plan(Q, N, nbits, k, mode);
    if (plan.kernel == RankKernel::none) return rank_refuse(what, plan, N, k);
    return rank2_launch(plan, q, blob_image(prepared, N, (nbits + 63) / 64, plan.kernel), nullptr, nullptr, nullptr, cum, Q, N, nbits, k,
                        0, (hipStream_t)stream, &apx);
}

extern "C" int wv_hamming_map_at_k(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab,
                                   int lwords, int Q, int64_t N, int nbits, int k, float *ap, int32_t *nrel, void *stream)
{
    WV_REQUIRE(lwords >= 1, "hamming_map_at_k: lwords=%d", lwords);
    if (lwords > 2) WV_FAIL(WV_ENOTSUP, "hamming_map_at_k: %d label words (more than 128 classes): wv_hamming_topk + wv_map_at_k", lwords);
    if (int rc = validate_rank_args("hamming_map_at_k", q && prepared && prepared_labels && qlab && ap, Q, N, nbits, k)) return rc;
    if (Q == 0) return WV_OK;
    const Rank2Ap apx{(const uint32_t *)prepared_labels, qlab, lwords, ap, nrel, nullptr, 0, 0};
    return fused_call("hamming_map_at_k", RankMode::ap, q, prepared, apx, nullptr, Q, N, nbits, k, stream);
}

// ---------------------------------------------------------------------------------- precision / recall by Hamming radius
extern "C" int wv_hamming_radius_hist(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab,
                                      int lwords, int Q, int64_t N, int nbits, uint32_t *cum, uint32_t *cumrel, void *stream)
{
    WV_REQUIRE(lwords >= 1, "hamming_radius_hist: lwords=%d", lwords);
    if (lwords > 2) WV_FAIL(WV_ENOTSUP, "hamming_radius_hist: %d label words (more than 128 classes)", lwords);
    if (int rc = validate_rank_shape("hamming_radius_hist", q && prepared && prepared_labels && qlab && cum && cumrel, Q, N, nbits)) return rc;
    if (Q == 0) return WV_OK;
    if (int rc = require_aligned16("hamming_radius_hist", "prepared", prepared)) return rc;
    if (int rc = require_aligned16("hamming_radius_hist", "prepared_labels", prepared_labels)) return rc;
    const RankPlan plan = rank_plan(Q, N, nbits, 0, RankMode::radius);
    if (plan.kernel == RankKernel::none) return rank_refuse("hamming_radius_hist", plan, N, 0);
    const Rank2Ap apx{(const uint32_t *)prepared_labels, qlab, lwords, nullptr, nullptr, nullptr, 0, 0};
    return rank2_radius_launch(plan, q, blob_image(prepared, N, (nbits + 63) / 64, plan.kernel), apx, cum, cumrel, Q, N, nbits,
                               (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------- sharded search, two steps
// 16-bit lists and / or histograms of one shard (RankMode::rows16, hist): windowed kernel, or WV_ENOTSUP
static int shard_call(const char *what, RankMode mode, const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows16,
                      uint32_t *cum, int Q, int64_t N, int nbits, int k, void *workspace, size_t workspace_bytes, void *stream)
{
    const RankPlan plan = rank_plan(Q, N, nbits, k, mode);
    if (plan.kernel == RankKernel::none) return rank_refuse(what, plan, N, k);
    if (int rc = require_aligned16(what, "prepared", prepared)) return rc;
    if (!prepared)
        if (int rc = require_workspace(what, workspace, workspace_bytes, Q, N, nbits, k)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const void *img = nullptr;
    if (int rc = rank_image(plan, db, prepared, workspace, N, (nbits + 63) / 64, st, &img)) return rc;
    return rank2_launch(plan, q, img, nullptr, rows16, nullptr, cum, Q, N, nbits, k, 0, st);
}

extern "C" int wv_hamming_hist(const uint64_t *q, const uint64_t *db, const void *prepared, uint32_t *cum, int Q, int64_t N,
                               int nbits, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_shape("hamming_hist", q && cum && (db || prepared), Q, N, nbits)) return rc;
    if (Q == 0) return WV_OK;
    return shard_call("hamming_hist", RankMode::hist, q, db, prepared, nullptr, cum, Q, N, nbits, 0, workspace, workspace_bytes, stream);
}

extern "C" int wv_hamming_shard_prefix(const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows, uint32_t *cum,
                                       int Q, int64_t N, int nbits, int k, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_args("hamming_shard_prefix", q && rows && cum && (db || prepared), Q, N, nbits, k)) return rc;
    if (Q == 0) return WV_OK;
    return shard_call("hamming_shard_prefix", RankMode::rows16, q, db, prepared, rows, cum, Q, N, nbits, k, workspace, workspace_bytes,
                      stream);
}

extern "C" int wv_hamming_shard_relbits(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab,
                                        int lwords, uint64_t *relbits, int64_t relbits_ld, uint32_t *cum, int64_t cum_ld, int Q,
                                        int64_t N, int nbits, int k, void *stream)
{
    WV_REQUIRE(lwords >= 1, "hamming_shard_relbits: lwords=%d", lwords);
    if (lwords > 2) WV_FAIL(WV_ENOTSUP, "hamming_shard_relbits: %d label words (more than 128 classes)", lwords);
    WV_REQUIRE((relbits_ld == 0 || relbits_ld >= (k + 63) / 64) && (cum_ld == 0 || cum_ld >= nbits + 2),
               "hamming_shard_relbits: row pitches %lld / %lld too small", (long long)relbits_ld, (long long)cum_ld);
    if (int rc = validate_rank_args("hamming_shard_relbits", q && prepared && prepared_labels && qlab && relbits && cum, Q, N, nbits, k))
        return rc;
    if (Q == 0) return WV_OK;
    const Rank2Ap apx{(const uint32_t *)prepared_labels, qlab, lwords, nullptr, nullptr, relbits, relbits_ld, cum_ld};
    return fused_call("hamming_shard_relbits", RankMode::relbits, q, prepared, apx, cum, Q, N, nbits, k, stream);
}

extern "C" int wv_merge_relbits_map(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q,
                                    int kin, int k, int nbits, float *ap, int32_t *nrel, int32_t *need_out, void *stream)
{
    WV_REQUIRE((relbits_ld == 0 || relbits_ld >= (kin + 63) / 64) && (cum_ld == 0 || cum_ld >= nbits + 2),
               "merge_relbits_map: row pitches %lld / %lld too small", (long long)relbits_ld, (long long)cum_ld);
    WV_REQUIRE(relbits && cum && ap, "merge_relbits_map: null buffer");
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1 && k >= 1, "merge_relbits_map: bad shape G=%d Q=%d kin=%d k=%d", G, Q, kin, k);
    if (int rc = require_nbits("merge_relbits_map", nbits)) return rc;
    if (Q == 0) return WV_OK;
    const int nbins = nbits + 1, w32 = 2 * (int)ceil_div(kin, 64), mwords = (k + 31) / 32 + 1;
    const size_t lds = ((size_t)G * (nbins + 1) + nbins + 1 + mwords + (mwords & 1) + ap_scratch_dwords<256>() + 4) * 4;
    WV_REQUIRE(lds <= 60 * 1024, "merge_relbits_map: too many shards (G=%d)", G);
    hipLaunchKernelGGL(k_merge_relbits_ap, dim3(Q), dim3(256), lds, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(relbits),
                       cum, G, Q, kin, w32, k, nbins, ap, nrel, need_out, relbits_ld ? 2 * relbits_ld : (int64_t)w32,
                       cum_ld ? cum_ld : (int64_t)(nbins + 1));
    WV_CHECK_LAUNCH("k_merge_relbits_ap");
    return WV_OK;
}

// ---------------------------------------------------------------------------------- average precision at several cut-offs
// The cut-offs of a call (HOST pointer): 1 .. WV_MAX_CUTOFFS of them, strictly ascending, inside [1, limit].
static int validate_cuts(const char *what, const int *ks, int nk, int64_t limit, const char *limit_name, ApCuts &cuts)
{
    static_assert(kMaxCutoffs == WV_MAX_CUTOFFS, "ap_walk.hpp and wvhash.h disagree");
    WV_REQUIRE(ks, "%s: null cut-off list", what);
    WV_REQUIRE(nk >= 1 && nk <= kMaxCutoffs, "%s: %d cut-offs (supported: 1..%d)", what, nk, kMaxCutoffs);
    cuts.n = nk;
    for (int i = 0; i < kMaxCutoffs; ++i) cuts.k[i] = i < nk ? ks[i] : 0;
    WV_REQUIRE(ks[0] >= 1, "%s: cut-off %d must be >= 1", what, ks[0]);
    for (int i = 1; i < nk; ++i)
        WV_REQUIRE(ks[i] > ks[i - 1], "%s: cut-offs must be strictly ascending (ks[%d]=%d after %d)", what, i, ks[i], ks[i - 1]);
    WV_REQUIRE(ks[nk - 1] <= limit, "%s: largest cut-off %d must be <= %s=%lld", what, ks[nk - 1], limit_name, (long long)limit);
    return WV_OK;
}

extern "C" int wv_hamming_map_at_ks(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab,
                                    int lwords, int Q, int64_t N, int nbits, const int *ks, int nk, float *ap, int32_t *nrel,
                                    void *stream)
{
    WV_REQUIRE(lwords >= 1, "hamming_map_at_ks: lwords=%d", lwords);
    if (lwords > 2) WV_FAIL(WV_ENOTSUP, "hamming_map_at_ks: %d label words (more than 128 classes): wv_hamming_topk + wv_map_at_ks", lwords);
    if (int rc = validate_rank_shape("hamming_map_at_ks", q && prepared && prepared_labels && qlab && ap, Q, N, nbits)) return rc;
    ApCuts cuts;
    if (int rc = validate_cuts("hamming_map_at_ks", ks, nk, N, "N", cuts)) return rc;
    if (Q == 0) return WV_OK;
    if (int rc = require_aligned16("hamming_map_at_ks", "prepared", prepared)) return rc;
    if (int rc = require_aligned16("hamming_map_at_ks", "prepared_labels", prepared_labels)) return rc;
    const int kmax = cuts.k[nk - 1];
    const RankPlan plan = rank_plan(Q, N, nbits, kmax, RankMode::ap);    // list, window, LDS and bitmap: sized by the largest cut-off
    if (plan.kernel == RankKernel::none)
        WV_FAIL(WV_ENOTSUP, "hamming_map_at_ks: %lld rows / largest cut-off %d %s; call wv_hamming_topk + wv_map_at_ks instead",
                (long long)N, kmax, plan.why);
    const Rank2Ap apx{(const uint32_t *)prepared_labels, qlab, lwords, ap, nrel, nullptr, 0, 0};
    return rank2_launch(plan, q, blob_image(prepared, N, (nbits + 63) / 64, plan.kernel), nullptr, nullptr, nullptr, nullptr, Q, N, nbits,
                        kmax, 0, (hipStream_t)stream, &apx, &cuts);
}

// dynamic LDS of k_merge_relbits_ap_cuts: run boundaries [G][nbins + 1], bin bases, the kmax-bit merged string, the walk's scratch
extern "C" size_t wv_merge_relbits_map_ks_lds_bytes(int G, int kmax, int nbits)
{
    if (G < 1 || kmax < 1 || nbits < 1 || nbits > 128) return 0;
    const int nbins = nbits + 1;
    const size_t mwords = (size_t)(kmax + 31) / 32 + 1;
    return ((size_t)G * (nbins + 1) + nbins + 1 + ap_cuts_scratch_dwords<256>() + 4) * 4 + (mwords + (mwords & 1)) * 4;
}

extern "C" int wv_merge_relbits_map_ks(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q,
                                       int kin, const int *ks, int nk, int nbits, float *ap, int32_t *nrel, int32_t *need_out,
                                       void *stream)
{
    WV_REQUIRE((relbits_ld == 0 || relbits_ld >= (kin + 63) / 64) && (cum_ld == 0 || cum_ld >= nbits + 2),
               "merge_relbits_map_ks: row pitches %lld / %lld too small", (long long)relbits_ld, (long long)cum_ld);
    WV_REQUIRE(relbits && cum && ap, "merge_relbits_map_ks: null buffer");
    WV_REQUIRE(G >= 1 && Q >= 0 && kin >= 1, "merge_relbits_map_ks: bad shape G=%d Q=%d kin=%d", G, Q, kin);
    if (int rc = require_nbits("merge_relbits_map_ks", nbits)) return rc;
    ApCuts cuts;
    if (int rc = validate_cuts("merge_relbits_map_ks", ks, nk, 0x7fffffff, "INT_MAX", cuts)) return rc;
    if (Q == 0) return WV_OK;
    const int kmax = cuts.k[nk - 1], nbins = nbits + 1, w32 = 2 * (int)ceil_div(kin, 64);
    const size_t lds = wv_merge_relbits_map_ks_lds_bytes(G, kmax, nbits), limit = WV_MERGE_RELBITS_LDS_LIMIT;
    if (lds > limit)
        WV_FAIL(WV_ENOTSUP, "merge_relbits_map_ks: the merged string of the largest cut-off %d does not fit LDS beside the run boundaries "
                "of G=%d shards (%zu bytes needed, %zu available)", kmax, G, lds, limit);
    hipLaunchKernelGGL(k_merge_relbits_ap_cuts, dim3(Q), dim3(256), lds, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(relbits),
                       cum, G, Q, kin, w32, nbins, ap, nrel, need_out, relbits_ld ? 2 * relbits_ld : (int64_t)w32,
                       cum_ld ? cum_ld : (int64_t)(nbins + 1), cuts);
    WV_CHECK_LAUNCH("k_merge_relbits_ap_cuts");
    return WV_OK;
}

extern "C" int wv_map_at_ks(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                            int lwords, float *ap, int32_t *nrel, void *stream)
{
    WV_REQUIRE(idx && qlab && dblab && ap, "map_at_ks: null buffer");
    WV_REQUIRE(Q >= 0 && lwords >= 1 && ld >= 1, "map_at_ks: bad shape Q=%d ld=%lld lwords=%d", Q, (long long)ld, lwords);
    ApCuts cuts;
    if (int rc = validate_cuts("map_at_ks", ks, nk, ld, "ld", cuts)) return rc;
    if (Q == 0) return WV_OK;
    hipStream_t st = (hipStream_t)stream;
    if (lwords == 1)
        hipLaunchKernelGGL((k_map_at_ks<1>), dim3(Q), dim3(256), 0, st, idx, ld, qlab, dblab, lwords, ap, nrel, cuts);
    else if (lwords == 2)
        hipLaunchKernelGGL((k_map_at_ks<2>), dim3(Q), dim3(256), 0, st, idx, ld, qlab, dblab, lwords, ap, nrel, cuts);
    else
        hipLaunchKernelGGL((k_map_at_ks<0>), dim3(Q), dim3(256), 0, st, idx, ld, qlab, dblab, lwords, ap, nrel, cuts);
    WV_CHECK_LAUNCH("k_map_at_ks");
    return WV_OK;
}

extern "C" int wv_hamming_topk_rows16(const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows, int Q,
                                      int64_t N, int nbits, int k, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_args("hamming_topk_rows16", q && rows && (db || prepared), Q, N, nbits, k)) return rc;
    if (Q == 0) return WV_OK;
    return shard_call("hamming_topk_rows16", RankMode::rows16, q, db, prepared, rows, nullptr, Q, N, nbits, k, workspace, workspace_bytes,
                      stream);
}
