// Batch mAP proxy for gfx950: average precision of every query over the inner-product ranking of a small database
// (N <= WV_IP_MAP_ROWS_MAX rows, D <= 512), scores, ranking and AP in ONE launch -- no [Q, k] list, no workspace.
//
// Reference: calculate_maphashing on real-valued embeddings (accuracy_calculator.py:203-231 with calc_hamming_dist :183-186,
// 0.5 * (nbits - q @ r.T)), as compute_batch_map calls it on a minibatch every training step (main/engine/batch_map.py).
//
// k_ip_map: one workgroup of 256 threads per query.
//   scores   thread t owns rows t, t + 256, ...: the database is staged through LDS 256 rows x 16 k-values at a time
//            (coalesced 64-byte row segments in, the next step's in registers while this one is computed; one odd-pitched
//            row per thread out: conflict-free), the query row is staged once, zero-padded to whole tiles.  A score is ONE
//            fmaf chain over k in the order wv_knn_float's matrix cores accumulate it (accumulation_order, host_knn.cpp):
//            8c + e, 8c + 4 + e for e = 0..3 of every chunk c of eight, starting from 0.0f -- the bits
//            wv_knn_float(metric IP) writes (v_mfma_f32_32x32x2_f32 is an fmaf chain; the zero padding adds exact zeros,
//            and a -0 it could turn into +0 has the same key).
//   ranking  64-bit words (order-preserving descending key << 32 | row) in LDS, padded to a power of two with all-ones
//            words (they sort behind every row), bitonic sort, two strides per pass: ascending word = descending score,
//            ties by ascending row.  The words are distinct, so the order is the one wv_knn_float's stable ranking produces.
//   AP       relevance bit of list position p = round * 256 + t from the label words, then the walk of ap_walk.hpp -- the
//            device code wv_map_at_k's arithmetic is defined by, at its 256 threads per query: the same bits.
// LDS: 16 KB list + 17 KB tile + 2 KB query + the walk's scratch = 36 KB, four workgroups per CU: a batch of 1024
// queries is resident at once on 256 CUs.
#include "common.hpp"
#include "ap_walk.hpp"
#include "ip_map.hpp"

namespace wv {

constexpr int kImThreads = 256;
constexpr int kImKc = 16;                     // k-values per staged tile: two chunks of the accumulation order
constexpr int kImPitch = kImKc + 1;           // odd: thread t reads row t of the tile, bank (17 t + k) % 32
static_assert(kIpMapMaxRows / kImThreads <= kApRounds, "the walk is one chunk of ap_walk.hpp");
static_assert(kIpMapMaxD % kImKc == 0 && kImKc % 8 == 0, "whole tiles, whole chunks of eight");

// VEC: D % 4 == 0 and db 16-byte aligned -- a step's values arrive as four 16-byte loads per thread, not sixteen 4-byte ones
template <bool VEC>
__global__ __launch_bounds__(kImThreads) void k_ip_map(const float *__restrict__ q, const float *__restrict__ db, int N, int D,
                                                       const uint64_t *__restrict__ qlab, const uint64_t *__restrict__ dblab,
                                                       int lwords, int k, int P, float *__restrict__ ap,
                                                       int32_t *__restrict__ nrel)
{
    constexpr int NW = kImThreads / 64;
    __shared__ uint64_t list[kIpMapMaxRows];
    __shared__ float tile[kImThreads * kImPitch];
    __shared__ __attribute__((aligned(16))) float qs[kIpMapMaxD];
    __shared__ uint32_t cnt[kApRounds * NW];
    __shared__ double wsum[NW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t qi = blockIdx.x;

    const int Dp = (D + kImKc - 1) / kImKc * kImKc;
    const float *qrow = q + qi * D;
    for (int j = t; j < Dp; j += kImThreads) qs[j] = j < D ? qrow[j] : 0.f;

    // One step = 256 rows x kImKc k-values.  The next step's values travel global -> registers while this step is computed:
    // kImKc loads per thread in flight across the step's barriers.
    const int nk = Dp / kImKc, steps = (N + kImThreads - 1) / kImThreads * nk;
    float reg[kImKc];
    // element j of a thread: row (j * 256 + t) / kImKc, column (j * 256 + t) % kImKc of the step; VEC: the same for groups of four
    auto fetch = [&](int row0, int k0) {
        if (VEC) {
#pragma unroll
            for (int j = 0; j < kImKc / 4; ++j) {
                const int flat = j * kImThreads + t, row = row0 + flat / (kImKc / 4), kk = k0 + flat % (kImKc / 4) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < N && kk < D) v = *reinterpret_cast<const float4 *>(db + (int64_t)row * D + kk);   // kk + 3 < D: D % 4 == 0
                reg[4 * j] = v.x, reg[4 * j + 1] = v.y, reg[4 * j + 2] = v.z, reg[4 * j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kImKc; ++j) {
                const int flat = j * kImThreads + t, row = row0 + flat / kImKc, kk = k0 + flat % kImKc;
                reg[j] = (row < N && kk < D) ? db[(int64_t)row * D + kk] : 0.f;
            }
        }
    };
    fetch(0, 0);
    float acc = 0.f;
    for (int s = 0, row0 = 0, kc = 0; s < steps; ++s) {
        __syncthreads();                                          // the previous step is read (first pass: qs is written)
#pragma unroll
        for (int j = 0; j < kImKc; ++j) {
            const int flat = (VEC ? j / 4 : j) * kImThreads + t;
            if (VEC) tile[(flat / (kImKc / 4)) * kImPitch + flat % (kImKc / 4) * 4 + j % 4] = reg[j];
            else tile[(flat / kImKc) * kImPitch + flat % kImKc] = reg[j];
        }
        __syncthreads();
        const bool last_kc = kc + 1 == nk;
        if (s + 1 < steps) fetch(last_kc ? row0 + kImThreads : row0, last_kc ? 0 : (kc + 1) * kImKc);
        const float *mine = tile + t * kImPitch;
        const float *qk = qs + kc * kImKc;
#pragma unroll
        for (int c8 = 0; c8 < kImKc; c8 += 8) {
            const float4 qa = *reinterpret_cast<const float4 *>(qk + c8);
            const float4 qb = *reinterpret_cast<const float4 *>(qk + c8 + 4);
            acc = fmaf(qa.x, mine[c8 + 0], acc);
            acc = fmaf(qb.x, mine[c8 + 4], acc);
            acc = fmaf(qa.y, mine[c8 + 1], acc);
            acc = fmaf(qb.y, mine[c8 + 5], acc);
            acc = fmaf(qa.z, mine[c8 + 2], acc);
            acc = fmaf(qb.z, mine[c8 + 6], acc);
            acc = fmaf(qa.w, mine[c8 + 3], acc);
            acc = fmaf(qb.w, mine[c8 + 7], acc);
        }
        if (last_kc) {                                            // uniform: the rows' chains are complete
            const int row = row0 + t;
            if (row < N) list[row] = ((uint64_t)float_to_key(acc, true) << 32) | (uint32_t)row;
            acc = 0.f;
            row0 += kImThreads;
            kc = 0;
        } else {
            ++kc;
        }
    }
    for (int i = N + t; i < P; i += kImThreads) list[i] = ~0ull;   // behind every row: a row's low word is below 2^32 - 1

    // Bitonic sort of P = 2^m words, ascending.  The sort is bound by LDS traffic and barriers, so two strides share a pass:
    // the four words base + {0, h, 2h, 3h} (h = stride / 2; same direction, bit `size` lies above both strides) take the
    // compare-exchanges of stride and of h in registers; an odd stride count leaves stride 1 to a pass of pairs.
    auto order = [](uint64_t &a, uint64_t &b, bool up) {
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
        a = up ? lo : hi;
        b = up ? hi : lo;
    };
    for (int size = 2; size <= P; size <<= 1) {
        int stride = size >> 1;
        for (; stride >= 2; stride >>= 2) {
            const int h = stride >> 1;
            __syncthreads();
            for (int i = t; i < (P >> 2); i += kImThreads) {
                const int base = ((i & ~(h - 1)) << 2) | (i & (h - 1));   // i with two zero bits inserted at h and stride
                const bool up = (base & size) == 0;
                uint64_t e0 = list[base], e1 = list[base + h], e2 = list[base + stride], e3 = list[base + stride + h];
                order(e0, e2, up);
                order(e1, e3, up);
                order(e0, e1, up);
                order(e2, e3, up);
                list[base] = e0;
                list[base + h] = e1;
                list[base + stride] = e2;
                list[base + stride + h] = e3;
            }
        }
        if (stride == 1) {
            __syncthreads();
            for (int i = t; i < (P >> 1); i += kImThreads) {
                uint64_t a = list[2 * i], b = list[2 * i + 1];
                order(a, b, ((2 * i) & size) == 0);
                list[2 * i] = a;
                list[2 * i + 1] = b;
            }
        }
    }
    __syncthreads();

    // relevance of the first k positions (all of them rows: k <= N), then wv_map_at_k's walk
    const uint64_t ql0 = qlab[qi * lwords], ql1 = lwords == 2 ? qlab[qi * lwords + 1] : 0ull;
    const int R = (k + kImThreads - 1) / kImThreads;               // <= kIpMapMaxRows / 256 rounds: one chunk
    uint32_t relbits = 0;
    for (int r = 0; r < R; ++r) {
        const int p = r * kImThreads + t;
        bool rel = false;
        if (p < k) {
            const uint64_t *dl = dblab + (int64_t)(uint32_t)list[p] * lwords;
            uint64_t any = ql0 & dl[0];
            if (lwords == 2) any |= ql1 & dl[1];
            rel = any != 0;
        }
        relbits |= (rel ? 1u : 0u) << r;
        const uint64_t m = __ballot(rel);
        if (lane == 0) cnt[r * NW + wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    ApState st;
    ap_accum<kImThreads>(relbits, cnt, R, 0, t, st);
    ap_final<kImThreads>(st, wsum, t, ap + qi, nrel ? nrel + qi : nullptr, [] { __syncthreads(); });
}

}  // namespace wv

extern "C" int wv_ip_map_at_k(const float *q, const float *db, int Q, int64_t N, int D, const uint64_t *qlab,
                              const uint64_t *dblab, int lwords, int k, float *ap, int32_t *nrel, void *stream)
{
    const int refused = wv::ip_map_args("ip_map_at_k", q, db, Q, N, D, qlab, dblab, lwords, k, ap);
    if (refused != WV_OK || Q == 0) return refused;
    int P = 1;
    while (P < N) P <<= 1;
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(db) & 15) == 0;
    hipLaunchKernelGGL(vec ? wv::k_ip_map<true> : wv::k_ip_map<false>, dim3((unsigned)Q), dim3(wv::kImThreads), 0,
                       (hipStream_t)stream, q, db, (int)N, D, qlab, dblab, lwords, k, P, ap, nrel);
    WV_CHECK_LAUNCH("ip_map_at_k");
    return WV_OK;
}
