"""NDCG from graded label overlap and precision at top-K: the two entries of the reference's second evaluator
(main/engine/DSCH/_utils.py, MyEval.__call__ :1020-1060) next to mAP, the PR curve and P@H<=2 (engine/radius_metrics.py).

The reference's NDCG (:551-574) builds a [Q, N] matrix of shared-class counts, a [Q, N] argsort and, per query, a sort of all
N gains for the ideal DCG.  Here the ideal DCG comes from a per-query histogram of the overlaps (wv_label_overlap_hist, at
most 129 bins) and the DCG from the graded gain at the k list positions only (wv_ndcg_at_ks); both have host twins with the
same bits.  Gains are 2^overlap - 1 in fp64: exact to an overlap of 53, rounded like the reference's int64 -> float64
conversion to 62; from 63 the reference's int64 overflows (2^64 - 1 is -1 there), so beyond 62 the fp64 value is the
definition and parity is not claimed.  Ties in the ranking are broken by ascending row (the reference: whatever its
unstable sort produces).

p_topK (:496-513) is relevant entries / K at each cut-off: the hit counts wv_hamming_map_at_ks already returns.
"""
import torch

from .. import _lib
from .backend import backend
from .hamming import MAX_CUTOFFS

LIST_BYTES_MAX = 256 << 20          # the ranked lists of one query chunk (int32 [chunk, k_max]) stay below 256 MB
P_TOPK_DEFAULT = (1, 100, 200, 300, 400, 500, 600, 700, 800, 900, 1000)


def ndcg_from_sums(dcg, idcg):
    """(dcg, idcg) float64 [Q, nk] of ndcg_at_ks -> NDCG float64 [nk]: the mean over ALL queries of dcg / idcg where
    idcg > 0 (a query no row shares a class with contributes 0, as in the reference).  Torch on the tables' device."""
    if dcg.dim() != 2 or dcg.shape != idcg.shape:
        raise ValueError("ndcg_from_sums: expected two [Q, nk] tables (ndcg_at_ks)")
    if dcg.shape[0] == 0:
        raise ZeroDivisionError("ndcg_from_sums: no queries")
    dcg, idcg = dcg.double(), idcg.double()
    live = idcg > 0
    ratio = torch.where(live, dcg / torch.where(live, idcg, torch.ones_like(idcg)), torch.zeros_like(dcg))
    # a TENSOR divisor: torch divides by a Python scalar on the GPU by multiplying with its reciprocal, which is an ulp off
    return ratio.sum(0) / torch.full((), float(dcg.shape[0]), dtype=torch.float64, device=dcg.device)


def _chunk(kmax):
    return max(1, LIST_BYTES_MAX // (4 * max(int(kmax), 1)))


def ndcg_sums_packed(Hm, lists_of, Q, qlp, rlp, ks):
    """(dcg, idcg) float64 [Q, len(ks)] for packed labels; lists_of(lo, hi) -> int32 [hi - lo, >= max(ks)] ranked lists of the
    queries lo..hi.  The queries go through in chunks whose lists stay below LIST_BYTES_MAX.  Hm: hamming or hamming_host."""
    hist = Hm.label_overlap_hist(qlp, rlp)
    step = _chunk(max(ks))
    parts = [Hm.ndcg_at_ks(lists_of(lo, min(Q, lo + step)), qlp[lo:lo + step], rlp, ks, hist=hist[lo:lo + step])
             for lo in range(0, Q, step)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _prepare(qF, rF, qL, rL, device, what_name):
    B = backend(device)
    q, r, ql, rl = (B.move(t) for t in (qF, rF, qL, rL))
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1] or ql.dim() != 2 or rl.dim() != 2 or ql.shape[1] != rl.shape[1] \
            or ql.shape[0] != q.shape[0] or rl.shape[0] != r.shape[0]:
        raise ValueError(f"{what_name}: expected [Q, D] / [N, D] features and [Q, classes] / [N, classes] multi-hot labels")
    if rl.shape[1] > 128:
        raise ValueError(f"{what_name}: at most 128 classes (got {rl.shape[1]})")
    if q.shape[0] == 0 or r.shape[0] == 0:
        raise ZeroDivisionError(f"{what_name}: no queries or no database rows")
    return B, q, r, ql, rl


def _ranker(B, q, r, what, kmax):
    """lists_of(lo, hi) for the ranking `what` of NDCG: 0 cosine, 1 Hamming, 2 squared L2."""
    if what == 1:
        nbits = q.shape[1]
        if nbits > 128:
            raise ValueError(f"NDCG(what=1): +-1 codes of at most 128 bits (got {nbits})")
        qp, rp = B.H.pack_codes(q), B.H.pack_codes(r)         # raises ValueError for anything but exactly +1 / -1
        db = B.H.PreparedDB(rp, nbits) if rp.shape[0] > B.H.SHARD_ROWS_MAX else rp
        return lambda lo, hi: B.H.hamming_topk(qp[lo:hi], db, nbits, kmax, want_dist=False)[0]
    if what not in (0, 2):
        raise ValueError(f"NDCG: what={what} (0 cosine, 1 Hamming, 2 Euclidean)")
    q, r = q.float(), r.float()
    if what == 0:                                             # rows normalised like the reference's cos()
        q, r = q / q.norm(dim=1, keepdim=True), r / r.norm(dim=1, keepdim=True)
    metric = _lib.WV_METRIC_IP if what == 0 else _lib.WV_METRIC_L2_SQUARED
    return lambda lo, hi: B.knn_float(r, q[lo:hi], kmax, metric)[1]


def ndcg_at(qF, rF, qL, rL, ks, what=1, device=None):
    """NDCG at several cut-offs from ONE ranking -> float64 [len(ks)] (on the device that computed it).  ks: positive ints,
    any order; a cut-off beyond the database clips at its size.  Arguments as NDCG."""
    B, q, r, ql, rl = _prepare(qF, rF, qL, rL, device, "ndcg_at")
    N = r.shape[0]
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise ValueError("ndcg_at: ks must be a non-empty sequence of positive ints")
    eff = [min(k, N) for k in ks]
    uniq = sorted(set(eff))
    qlp, rlp = B.H.pack_labels(ql), B.H.pack_labels(rl)
    lists_of = _ranker(B, q, r, what, uniq[-1])
    cols = {}
    for s in range(0, len(uniq), MAX_CUTOFFS):
        part = uniq[s:s + MAX_CUTOFFS]
        vals = ndcg_from_sums(*ndcg_sums_packed(B.H, lists_of, q.shape[0], qlp, rlp, part))
        cols.update({k: vals[i] for i, k in enumerate(part)})
    return torch.stack([cols[k] for k in eff])


def NDCG(qF, rF, qL, rL, what=0, k=-1, device=None):
    """The reference's NDCG (DSCH/_utils.py:551-574), same name and argument order -> float.
    what: 0 cosine (rows normalised, inner-product k-NN), 1 Hamming (+-1 codes of at most 128 bits, exactly +1 / -1),
    2 squared Euclidean; k < 0 or k > N means N.  device='cpu': the host twins and nothing else; anything else: the GPU
    (WvhashUnavailable without one -- never a silent fallback)."""
    N = rF.shape[0]
    if k < 0 or k > N:
        k = N
    return float(ndcg_at(qF, rF, qL, rL, [int(k)], what=what, device=device)[0].item())


def p_topK(qB, rB, qL, rL, K=None, device=None):
    """The reference's p_topK (DSCH/_utils.py:496-513), same name, argument order and default K list -> float64 [len(K)]:
    at each min(K_i, N) the relevant entries among the K_i nearest rows / that number, mean over ALL queries.  The counts are
    the nrel column of wv_hamming_map_at_ks (where that kernel does not cover the shape: hamming_topk + map_at_ks); float64
    from exact integers."""
    B, q, r, ql, rl = _prepare(qB, rB, qL, rL, device, "p_topK")
    Hm = B.H
    K = list(P_TOPK_DEFAULT) if K is None else [int(x) for x in K]
    if not K or min(K) < 1:
        raise ValueError("p_topK: K must be a non-empty sequence of positive ints")
    (Q, nbits), N = q.shape, r.shape[0]
    if nbits > 128:
        raise ValueError(f"p_topK: +-1 codes of at most 128 bits (got {nbits})")
    eff = [min(x, N) for x in K]                              # clamp, de-duplicate for the call, map back below
    uniq = sorted(set(eff))
    qp, rp = Hm.pack_codes(q), Hm.pack_codes(r)
    qlp, rlp = Hm.pack_labels(ql), Hm.pack_labels(rl)
    db, labels = Hm.PreparedDB(rp, nbits), Hm.PreparedLabels(rlp)
    cols = {}
    for s in range(0, len(uniq), MAX_CUTOFFS):
        part = uniq[s:s + MAX_CUTOFFS]
        got = Hm.hamming_map_at_ks(qp, db, labels, qlp, nbits, part)      # None: outside the fused kernel (always, on the host)
        if got is not None:
            nrel = got[1]
        else:
            step = _chunk(part[-1])
            nrel = torch.cat([Hm.map_at_ks(Hm.hamming_topk(qp[lo:lo + step], db, nbits, part[-1], want_dist=False)[0],
                                           qlp[lo:lo + step], rlp, part)[1] for lo in range(0, Q, step)])
        cols.update({k: nrel[:, i].long().sum() for i, k in enumerate(part)})      # exact integers
    hits = torch.stack([cols[k] for k in eff]).double()
    # one correctly rounded division per cut-off (a tensor divisor: a scalar one becomes a reciprocal multiply on the GPU),
    # so that the GPU and device='cpu' return the same bits
    return hits / torch.tensor([float(k) * Q for k in eff], dtype=torch.float64, device=hits.device)
