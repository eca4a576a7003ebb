"""Shared by tests/test_ndcg_reference.py, tests/test_host_ndcg.py, tests/test_gpu_ndcg.py and tests/golden/make_golden_ndcg.py:
a plain numpy restatement of NDCG / precision at top-K as include/wvhash.h defines them, the exact interval that orderings
differing only inside distance buckets can produce, seeded inputs, the loader of the reference-made fixture
tests/golden/ndcg_golden.npz (data only) and the derived tolerances."""
import os

import numpy as np
import torch

HAMMING_CASES = ["c16_q9_n70_k5", "c32_q16_n300_k12", "c48_q24_n500_k38", "c64_q32_n1000_k38", "c128_q40_n777_k80", "far_q9_n70_k5",
                 "dense_q8_n120_k20", "two_q10_n150_k100"]
SHARED_WITH_RADIUS = HAMMING_CASES[:6]                        # inputs live in tests/golden/radius_golden.npz (same cases)
REAL_CASES = ["cos_q12_n200_d24", "l2_q12_n200_d24"]          # tie-free: what = 0 and what = 2
P_TOPK_K = [1, 5, 50, None]                                   # None = N


def ndcg_ks(N):
    """The cut-offs every fixture case stores (k = -1 means N)."""
    return [1, 7, 50, N // 2, -1]


def ndcg_tol(k):
    """Absolute tolerance on an NDCG value (<= 1) against the reference's arithmetic.  u = 2^-53; gains are exact; each of
    our terms carries <= 2 roundings (the reciprocal in w, the fma), the reference's 1 (the division); a sum of n
    non-negative terms adds <= (n - 1) u in any order.  So DCG and IDCG each differ by <= (2 n + 1) u relative, their ratio
    by <= (4 n + 2) u: (k + 2) * 2^-51 covers it, per query and for the mean."""
    return (k + 2) * 2.0 ** -51


def sum_tol(k):
    """Relative tolerance on ONE sum (DCG or IDCG) of k terms against the restatement: (2 k + 1) u, see ndcg_tol."""
    return (2 * k + 1) * 2.0 ** -53


def mean_tol(Q):
    """Two evaluations of the SAME per-query sums whose mean over Q ratios <= 1 is taken in another order (torch on another
    device, another table shape): (Q - 1) u for the order, and the roundings of the ratio and of the final division."""
    return (Q + 2) * 2.0 ** -53


def ptopk_tol(Q):
    """p_topK: the reference divides once in fp32 per query and cut-off and sums Q values <= 1 in fp32."""
    return (Q + 3) * 2.0 ** -24


def gains(rel):
    """2^rel - 1 as float64 (ldexp(1, rel) - 1: no int64 overflow, the definition above an overlap of 62)."""
    return np.ldexp(1.0, np.asarray(rel, dtype=np.int64).astype(np.int32)) - 1.0


def overlaps(ql, rl):
    """[Q, N] shared classes of 0/1 labels (exact small integers)."""
    return (np.asarray(ql, dtype=np.int64) @ np.asarray(rl, dtype=np.int64).T)


def dcg_sums(rank, Rel, k):
    """The definitions, per query: (dcg, idcg) float64 [Q].  rank: int [Q, >= k] row numbers (< 0: absent, contributes 0);
    Rel: [Q, N] overlaps.  Terms are gain / log2(p + 2) summed by numpy, the ideal list is a full descending sort."""
    Rel = np.asarray(Rel)
    Q, N = Rel.shape
    D = np.log2(2.0 + np.arange(k))
    dcg, idcg = np.zeros(Q), np.zeros(Q)
    for q in range(Q):
        r = np.asarray(rank[q][:k], dtype=np.int64)
        g = np.where(r >= 0, gains(Rel[q][np.maximum(r, 0)]), 0.0)
        dcg[q] = (g / D[:len(g)]).sum()
        best = np.sort(gains(Rel[q]))[::-1][:k]
        idcg[q] = (best / D[:len(best)]).sum()
    return dcg, idcg


def ndcg_restated(rank, Rel, k):
    """Mean over ALL queries of dcg / idcg where idcg > 0."""
    dcg, idcg = dcg_sums(rank, Rel, k)
    return float(np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0).sum() / len(dcg))


def canonical_order(d):
    """Ascending distance, ties by ascending row: what wv_hamming_topk and wv_knn_float return."""
    return np.argsort(np.asarray(d), axis=1, kind="stable")


def ndcg_tie_bounds(d, Rel, k):
    """(lo, hi): the exact interval of NDCG@k over all orderings that sort by d and differ only inside buckets of equal d.
    Complete buckets: gains descending for hi, ascending for lo; the bucket the cut falls into contributes its largest
    resp. smallest gains (the same lexicographic sort does both)."""
    d, Rel = np.asarray(d), np.asarray(Rel)
    Q, N = Rel.shape
    k = min(k, N)
    D = np.log2(2.0 + np.arange(k))
    lo = hi = 0.0
    for q in range(Q):
        g = gains(Rel[q])
        best = (np.sort(g)[::-1][:k] / D).sum()
        if best > 0:
            up = np.lexsort((-g, d[q]))[:k]
            dn = np.lexsort((g, d[q]))[:k]
            hi += (g[up] / D).sum() / best
            lo += (g[dn] / D).sum() / best
    return lo / Q, hi / Q


def ptopk_tie_bounds(d, relevant, K):
    """(lo, hi) float64 [len(K)]: the interval of the mean precision at min(K_i, N) over the same orderings.  Every number of
    kept relevant rows between the two extremes of the cut bucket is possible."""
    d, relevant = np.asarray(d), np.asarray(relevant).astype(bool)
    Q, N = relevant.shape
    lo, hi = np.zeros(len(K)), np.zeros(len(K))
    for i, kk in enumerate(K):
        t = min(kk, N)
        for q in range(Q):
            srt = np.sort(d[q])
            edge = srt[t - 1]                                  # the bucket the cut falls into
            inside = d[q] < edge
            bucket = d[q] == edge
            take = t - int(inside.sum())
            m, c = int(bucket.sum()), int((bucket & relevant[q]).sum())
            base = int((inside & relevant[q]).sum())
            lo[i] += (base + max(0, take - (m - c))) / t
            hi[i] += (base + min(c, take)) / t
    return lo / Q, hi / Q


def hamming_np(q, r):
    """[Q, N] integer Hamming distances of +-1 codes."""
    q, r = np.asarray(q, dtype=np.int64), np.asarray(r, dtype=np.int64)
    return (q.shape[1] - q @ r.T) // 2


def make_labels(Q, N, classes, p, seed):
    """Seeded multi-hot labels for the kernel tests: query 0 has no class, query 1 (when there is one) every class; row 0
    carries every class, row 1 (when there is one) none."""
    g = torch.Generator().manual_seed(seed)
    ql = (torch.rand(Q, classes, generator=g) < p).float()
    rl = (torch.rand(N, classes, generator=g) < p).float()
    ql[0] = 0
    if Q > 1:
        ql[1] = 1
    rl[0] = 1
    if N > 1:
        rl[1] = 0
    return ql, rl


def load_golden(golden_dir, name):
    """-> dict: q, r (float32 torch: +-1 codes or real features), ql, rl (float 0/1), order (int32 numpy [Q, cols]: the
    reference's own argsort, first `cols` columns), ks, ref_ndcg (float64, one per k), and for the Hamming cases K, ref_ptopk."""
    z = np.load(os.path.join(golden_dir, "ndcg_golden.npz"))
    out = {"order": z[f"{name}/order"], "ks": [int(x) for x in z[f"{name}/ks"]], "ref_ndcg": z[f"{name}/ref_ndcg"],
           "what": int(z[f"{name}/what"][0])}
    if name in SHARED_WITH_RADIUS:
        import radius_cases
        have = radius_cases.load_golden(golden_dir, name)
        out.update({key: have[key] for key in ("q", "r", "ql", "rl")})
        out.update({"K": [int(x) for x in z[f"{name}/K"]], "ref_ptopk": z[f"{name}/ref_ptopk"].astype(np.float64)})
        return out
    out.update({"ql": torch.from_numpy(z[f"{name}/ql"]).float(), "rl": torch.from_numpy(z[f"{name}/rl"]).float()})
    if out["what"] == 1:
        nbits = int(z[f"{name}/nbits"][0])
        unpack = lambda a: torch.from_numpy(np.unpackbits(a, axis=1)[:, :nbits].astype(np.float32)) * 2 - 1
        out.update({"q": unpack(z[f"{name}/q"]), "r": unpack(z[f"{name}/r"]), "K": [int(x) for x in z[f"{name}/K"]],
                    "ref_ptopk": z[f"{name}/ref_ptopk"].astype(np.float64)})
    else:
        out.update({"q": torch.from_numpy(z[f"{name}/q"]), "r": torch.from_numpy(z[f"{name}/r"])})
    return out


def scores_np(case):
    """[Q, N] float64 ranking keys of a fixture case, ascending = nearer (the reference's own formulas on its inputs)."""
    q, r = case["q"].double().numpy(), case["r"].double().numpy()
    if case["what"] == 1:
        return hamming_np(q, r).astype(np.float64)
    if case["what"] == 0:
        qn, rn = q / np.linalg.norm(q, axis=1)[:, None], r / np.linalg.norm(r, axis=1)[:, None]
        return 1.0 - qn @ rn.T
    return (q * q).sum(1)[:, None] - 2.0 * q @ r.T + (r * r).sum(1)[None, :]


HIST_N = [1, 63, 64, 65, 257, 1000, 4099]
HIST_Q = [1, 7, 33]
HIST_CLASSES = [5, 38, 64, 80, 128]
WALK_KS = [1, 63, 64, 255, 256, 257, 511, 1000]               # and N


def random_lists(Q, N, ld, seed, absent=0):
    """int32 [Q, ld] lists of distinct rows in random order (the walk does not care how they were ranked); `absent`: that
    many entries per query set to -1."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(N, generator=g)[:ld] for _ in range(Q)]).int()
    for q in range(Q):
        idx[q, torch.randperm(ld, generator=g)[:min(absent, ld)]] = -1
    return idx


def assert_sums_close(got, want, k, what):
    """dcg or idcg [Q] against the restatement: relative sum_tol(k)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(np.isfinite(got)), what
    assert np.all(np.abs(got - want) <= sum_tol(k) * np.abs(want)), (what, k, float(np.abs(got - want).max()))
