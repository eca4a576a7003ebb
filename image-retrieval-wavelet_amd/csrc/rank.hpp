// Hamming ranking, host side: which kernel ranks a shape and what it needs (the planner), where each kernel's database
// image lies in a prepared blob, and the interface between topk.hip (entry points, column kernel) and rank2.hip
// (windowed kernel).  Every fit rule lives in rank_plan(): the entry points ask it and launch what it answers.
#pragma once
#include "common.hpp"

namespace wv {

struct ApCuts;                               // ap_cuts.hpp

constexpr int kTopkThreads = 256;            // threads per workgroup of every ranking kernel
constexpr int kMaxBins = 130;                // nbits <= 128 (+1 bin for the padding value of ragged shard lists)
constexpr int kWinBins = 32;                 // windowed kernel: distance bins per window
constexpr int kWinRows = kWinBins + 1;       // + the dummy row
constexpr size_t kRankLdsLimit = 100 * 1024; // dynamic LDS a windowed workgroup may ask for

enum class RankKernel {
    none,        // no kernel takes the shape in this mode: RankPlan::why says which rule refused it
    column,      // first-generation column kernel (topk.hip): any N, any k
    window256,   // windowed kernel, 256 threads per query: N <= kImg256MaxRows
    window64,    // windowed kernel, one wave per query, 4 queries per workgroup: N <= kImg64MaxRows
};

// what the call wants from the ranking
enum class RankMode {
    lists,       // int32 lists, optional distance rows / histograms (wv_hamming_topk*): falls back to the column kernel
    rows16,      // 16-bit local row numbers (+ histograms): windowed kernel only
    hist,        // histograms only (k = 0): windowed kernel only
    ap,          // average precision of the list, never written (wv_hamming_map_at_k): windowed kernel only
    relbits,     // relevance string of the list (wv_hamming_shard_relbits): windowed kernel only
    radius,      // histograms of all rows and of the relevant rows (wv_hamming_radius_hist): 256-thread windowed kernel only
};

// a database image of the windowed kernel exists for databases (shards) of at most this many rows: one wave per query
// takes C <= 64 items per lane, 256 threads per query C <= 128 (distances cached in registers, 16-bit item numbers)
constexpr int64_t kImg64MaxRows = 64 * 64;
constexpr int64_t kImg256MaxRows = 256 * 128;

// the code width every Hamming ranking and merge entry point takes (topk.hip, merge.hip)
inline int require_nbits(const char *what, int nbits)
{
    WV_REQUIRE(nbits >= 1 && nbits <= 128, "%s: nbits=%d (supported: 1..128)", what, nbits);
    return WV_OK;
}

// threads that share one query
constexpr int rank_threads_per_query(RankKernel kern) { return kern == RankKernel::window64 ? 64 : 256; }

struct RankPlan {
    RankKernel kernel;
    int C;              // items per thread: ceil(N / threads per query)
    int NC;             // windowed kernel: distance-cache words of the instantiation (4 items each, C <= 4 * NC)
    size_t lds;         // dynamic LDS bytes of the launch
    const char *why;    // kernel == none: the rule that refused the shape ...
    const char *instead;  // ... and what to call instead (or "")
};

// words of the relevance bitmap: one bit per database row
__host__ __device__ inline int rank2_bitmap_words(int64_t N) { return (int)((N + 31) / 32); }

// LDS of one query of the windowed kernel (layout: Rank2Lds in rank2.hip)
inline size_t window_lds_bytes_per_query(int tpq, int k, int bm_words = 0)
{
    size_t b = (size_t)kWinRows * (tpq / 2) * 4;                 // table
    b += ((size_t)(k + tpq) * 2 + 15) / 16 * 16;                 // stage
    b += (size_t)(kMaxBins + 1 + kWinBins + 4 + 3) / 4 * 4 * 4;  // gbase, tot, misc
    b += (size_t)bm_words * 4;                                   // relevance bitmap
    b = (b + 15) / 16 * 16;
    const size_t hist = (size_t)(kMaxBins + 1) * 17 * 4;         // histogram-only mode: [bins + 1][16] dwords + totals
    return b > hist ? b : (hist + 15) / 16 * 16;
}

// LDS of the radius-histogram kernel (k_rank_radius, rank2.hip): count table [kMaxBins + 1][16] dwords (a dword = the cell of
// 16 threads: all rows in the low half, relevant rows in the high half), the two rows of totals, and the relevance bitmap
// over every ITEM number of the 256 threads (8 C words: padding items index it too) + the word a 64-bit read may touch
constexpr int rank_radius_bitmap_words(int C) { return 8 * C + 1; }
inline size_t radius_lds_bytes(int C)
{
    const size_t b = (size_t)(kMaxBins + 1) * 16 * 4 + (size_t)2 * (kMaxBins + 1) * 4 + (size_t)rank_radius_bitmap_words(C) * 4;
    return (b + 15) / 16 * 16;
}

// LDS of the column kernel: hist[nbins][256] (u16 pairs when N < 65536), tot[kMaxBins], base[kMaxBins + 1], misc[4]
inline bool column_u16(int64_t n_items) { return n_items < 65536; }
inline size_t column_lds_bytes(int nbins, bool u16)
{
    const size_t h = (size_t)nbins * (u16 ? kTopkThreads / 2 : kTopkThreads);
    return (h + kMaxBins + kMaxBins + 1 + 4 + 3) / 4 * 4 * sizeof(uint32_t);
}

inline RankPlan rank_plan_column(int64_t N, int nbits)
{
    return {RankKernel::column, (int)ceil_div(N, kTopkThreads), 0, column_lds_bytes(nbits + 1, column_u16(N)), nullptr, ""};
}

// The windowed kernel for lists of k entries from N rows, or none.  WV_TOPK_V2 (diagnostic library): "0" = never,
// "64" / "256" = pin the variant (tests, tuning); a pinned variant that does not fit the shape is ignored.
inline RankKernel rank_window_kernel(int Q, int64_t N, int k)
{
    const char *force = ::wv::tune("WV_TOPK_V2");
    if (force && force[0] == '0') return RankKernel::none;
    if (N >= 65536 || 2 * (k + 128) >= 65536) return RankKernel::none;   // list cells count bytes in 16 bits
    const bool fits256 = N <= kImg256MaxRows && window_lds_bytes_per_query(256, k) <= kRankLdsLimit;
    const bool fits64 = N <= kImg64MaxRows && 4 * window_lds_bytes_per_query(64, k) <= kRankLdsLimit;
    if (force && atoi(force) == 64 && fits64) return RankKernel::window64;
    if (force && atoi(force) == 256 && fits256) return RankKernel::window256;
    // one wave per query pays when each query has little work and there are enough queries to fill the chip
    if (fits64 && Q >= 4096) return RankKernel::window64;
    return fits256 ? RankKernel::window256 : (fits64 ? RankKernel::window64 : RankKernel::none);
}

// THE rule: which kernel ranks Q queries against N rows of nbits-bit codes for lists of k entries (hist: k = 0).
inline RankPlan rank_plan(int Q, int64_t N, int nbits, int k, RankMode mode)
{
    const bool fused = mode == RankMode::ap || mode == RankMode::relbits;
    const char *instead = mode == RankMode::ap ? "; call wv_hamming_topk + wv_map_at_k instead" : "";
    RankKernel kern = rank_window_kernel(Q, N, std::max(k, 1));
    if (kern == RankKernel::none) {
        if (mode == RankMode::lists) return rank_plan_column(N, nbits);
        return {RankKernel::none, 0, 0, 0, "are outside the windowed kernel (rows <= 32768, 16-bit row numbers: 2 (k + 128) < 65536)",
                instead};
    }
    // the AP walk keeps 32 list positions per thread (N <= kImg64MaxRows here: the 256-thread image exists and fits)
    if (fused && kern == RankKernel::window64 && k > 32 * 64) kern = RankKernel::window256;
    // the radius histograms exist for 256 threads per query only (N <= kImg256MaxRows here: that image exists)
    if (mode == RankMode::radius) kern = RankKernel::window256;
    RankPlan p{kern, 0, 0, 0, nullptr, ""};
    const int tpq = rank_threads_per_query(kern);
    p.C = (int)ceil_div(N, tpq);
    p.NC = p.C <= 16 ? 4 : (p.C <= 32 ? 8 : (p.C <= 64 ? 16 : (p.C <= 100 ? 25 : 32)));
    p.lds = window_lds_bytes_per_query(tpq, k, fused ? rank2_bitmap_words(N) : 0) * (kTopkThreads / tpq);
    if (mode == RankMode::radius) p.lds = radius_lds_bytes(p.C);
    if (fused && p.lds > kRankLdsLimit)
        return {RankKernel::none, 0, 0, 0, "do not fit the fused kernel's LDS (list + relevance bitmap)", instead};
    return p;
}

// WV_ENOTSUP for a plan without a kernel
inline int rank_refuse(const char *what, const RankPlan &p, int64_t N, int k)
{
    WV_FAIL(WV_ENOTSUP, "%s: %lld rows / k=%d %s%s", what, (long long)N, k, p.why, p.instead);
}

// ---- database images.  Prepared blob = [distance-kernel tile image | column image | window256 image (N <= kImg256MaxRows) |
// window64 image (N <= kImg64MaxRows)], every image 256-byte aligned; the ranking images exist for codes of <= 2 words.
inline size_t rank_image_bytes(RankKernel kern, int64_t N, int words)
{
    if (kern == RankKernel::column) return (size_t)ceil_div(N, kTopkThreads) * kTopkThreads * words * sizeof(uint64_t);
    const int tpq = rank_threads_per_query(kern);                // 16 bytes per (row, thread): two 64-bit codes or one 128-bit
    const int64_t C = ceil_div(N, tpq), rows = words == 1 ? (C + 1) / 2 : C;
    return (size_t)rows * tpq * 16;
}

struct BlobLayout {
    size_t column, window256, window64, total;                   // byte offsets of the images (an absent one has no bytes)
};
inline BlobLayout blob_layout(int64_t N, int words)
{
    BlobLayout L;
    L.column = L.window256 = L.window64 = L.total = (size_t)align_up((int64_t)dist_prepared_bytes(N, words), 256);
    if (words > 2) return L;
    L.window256 = L.column + (size_t)align_up((int64_t)rank_image_bytes(RankKernel::column, N, words), 256);
    L.window64 = L.window256 + (N <= kImg256MaxRows ? (size_t)align_up((int64_t)rank_image_bytes(RankKernel::window256, N, words), 256) : 0);
    L.total = L.window64 + (N <= kImg64MaxRows ? rank_image_bytes(RankKernel::window64, N, words) : 0);
    return L;
}
// the image a plan's kernel reads inside a prepared blob
inline const void *blob_image(const void *prepared, int64_t N, int words, RankKernel kern)
{
    const BlobLayout L = blob_layout(N, words);
    return (const char *)prepared + (kern == RankKernel::column ? L.column : (kern == RankKernel::window256 ? L.window256 : L.window64));
}

// ---- rank2.hip
// builds the image of a windowed kernel (RankKernel::window256 / window64)
int rank2_prepare(const uint64_t *db, void *img, int64_t N, int words, RankKernel kern, hipStream_t st);
size_t rank2_labels_bytes(int64_t N, int lwords);
int rank2_labels_prepare(const uint64_t *dblab, void *cls, int64_t N, int lwords, hipStream_t st);

// average precision instead of the list (RankMode::ap / relbits)
struct Rank2Ap {
    const uint32_t *cls;     // class-major label bit matrix [64 * lwords][ceil(N / 32)] (rank2_labels_prepare)
    const uint64_t *qlab;    // [Q][lwords] label words of every query
    int lwords;              // 1 or 2 (up to 128 classes)
    float *ap;               // [Q]
    int32_t *nrel;           // [Q] relevant entries among the k (or NULL)
    uint64_t *relbits;       // [Q][ceil(k / 64)] instead of ap: the relevance string of the list (sharded mAP)
    int64_t relbits_ld;      // row pitch of relbits in uint64 (0 = ceil(k / 64))
    int64_t cum_ld;          // row pitch of the histograms in uint32 (0 = nbits + 2): relbits and cum may share one wire buffer
};

// Launches the windowed kernel of `plan` (window256 / window64) on its image `img`.  idx (int32 global indices) or rows16
// (16-bit local row numbers) receives the list; k == 0: histogram only; apx: RankMode::ap / relbits, NULL otherwise.
// cuts (RankMode::ap only): average precision at several cut-offs, k = the largest, apx->ap / nrel are [Q][cuts->n].
int rank2_launch(const RankPlan &plan, const uint64_t *q, const void *img, int32_t *idx, uint16_t *rows16, uint8_t *dist,
                 uint32_t *cum, int Q, int64_t N, int nbits, int k, int64_t idx_offset, hipStream_t st,
                 const Rank2Ap *apx = nullptr, const ApCuts *cuts = nullptr);

// Launches the radius-histogram kernel of `plan` (RankMode::radius: window256) on its image: cum / cumrel uint32 [Q][nbits + 2],
// rows (cumrel: rows sharing a label bit with the query) with distance < b.  apx: cls, qlab, lwords are read.
int rank2_radius_launch(const RankPlan &plan, const uint64_t *q, const void *img, const Rank2Ap &apx, uint32_t *cum, uint32_t *cumrel,
                        int Q, int64_t N, int nbits, hipStream_t st);

}  // namespace wv
