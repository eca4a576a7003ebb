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
// kernel (rank2.hip); rank_plan() (rank.hpp) decides which.  The file also holds the ranking, prepare, fused and shard
// entry points.  The merges of the shards' results: merge.hip; the metrics over written lists: list_ap.hip.
#include "rank.hpp"
#include "ap_cuts.hpp"

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

extern "C" int wv_hamming_topk_rows16(const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows, int Q,
                                      int64_t N, int nbits, int k, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate_rank_args("hamming_topk_rows16", q && rows && (db || prepared), Q, N, nbits, k)) return rc;
    if (Q == 0) return WV_OK;
    return shard_call("hamming_topk_rows16", RankMode::rows16, q, db, prepared, rows, nullptr, Q, N, nbits, k, workspace, workspace_bytes,
                      stream);
}
