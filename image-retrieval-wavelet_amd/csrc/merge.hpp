// The dynamic LDS of the merge kernels (merge.hip), stated once: the kernels carve their arrays from it, the entry points
// and wv_merge_relbits_map_ks_lds_bytes size their launches from it, and one gate holds it against
// WV_MERGE_RELBITS_LDS_LIMIT.
#pragma once
#include "ap_walk.hpp"

namespace wv {

// Offsets in dwords from the start of the workgroup's dynamic LDS:
//   start  [G][nbins + 1]  first position of shard g's list with distance >= b
//   delta  [G][nbins]      list merges only: entry p of shard g, distance b, goes to output position p + delta[g][b]
//   base   [nbins + 1]     entries of all shards with distance < b
//   string                 relevance-string merges only: k bits + the word a shifted copy may spill into, padded to 8 bytes
//   scratch                relevance-string merges only: the walk's (ap_cuts_scratch_dwords<256>(); the single-cut walk uses less)
//   slack                  kSlack dwords nothing addresses: the launches have always asked for them, and the sizes are pinned
//   end                    the dwords a launch asks for
// I: the integer the offsets are computed in -- int in the kernels (a launch that passed the gate fits 60 KB), int64_t on
// the host, which must size any G and k before it can refuse them.
template <typename I>
struct MergeLayout {
    static constexpr int kSlack = 4;
    I start, delta, base, string, string_words, scratch, slack, end;   // string_words: dwords of the string before the padding
    WV_HD size_t bytes() const { return (size_t)end * 4; }

    // k_merge_sorted, k_merge_cum
    WV_HD static MergeLayout lists(I G, I nbins)
    {
        MergeLayout L;
        L.start = 0;
        L.delta = G * (nbins + 1);
        L.base = L.delta + G * nbins;
        L.string = L.scratch = L.slack = L.base + nbins + 1;
        L.string_words = 0;
        L.end = L.slack + kSlack;
        return L;
    }
    // k_merge_relbits_ap, k_merge_relbits_ap_cuts: the string of the (largest) cut-off k
    WV_HD static MergeLayout relbits(I G, I nbins, I k)
    {
        MergeLayout L;
        L.start = 0;
        L.delta = L.base = G * (nbins + 1);
        L.string = L.base + nbins + 1;
        L.string_words = (k + 31) / 32 + 1;
        L.scratch = L.string + L.string_words + (L.string_words & 1);
        L.slack = L.scratch + ap_cuts_scratch_dwords<256>();
        L.end = L.slack + kSlack;
        return L;
    }
};

}  // namespace wv
