"""Precision and recall by Hamming radius: what a hash-table lookup within radius r returns and how much of it is relevant.

The reference's vendored evaluator computes them from a [Q, N] distance matrix and a [Q, N] relevance matrix
(main/engine/DSCH/_utils.py: pr_curve :469-493, get_precision_recall_by_Hamming_Radius :577-594).  Both are functions of
two small integer tables per query -- rows at distance < b, and those of them that share a label with the query
(wv_hamming_radius_hist / its host twin, include/wvhash.h) -- which is all that is built here.  The arithmetic on the
[Q, nbits + 2] tables is torch on the tables' device, float64 from exact integers.
"""
import torch

from .backend import backend
from .hamming import SHARD_ROWS_MAX


def _tables(cum, cumrel):
    if cum.dim() != 2 or cum.shape != cumrel.shape or cum.shape[1] < 3:
        raise ValueError("radius metrics: expected two [Q, nbits + 2] tables (hamming_radius_hist)")
    return cum.double(), cumrel.double(), cum.shape[1] - 2


def radius_curves(cum, cumrel):
    """(cum, cumrel) of hamming_radius_hist -> (P, R) float64 [nbits + 1]: precision and recall at every radius 0..nbits by
    the rule of pr_curve (:469-493).  Per query with a relevant row and radius r: p = relevant found / found (0.1 stands in
    for "found nothing"), r = relevant found / relevant rows; a query without relevant rows contributes zeros; every column
    of P and of R is divided by the number of queries with p > 0 at that radius (0.1 when there is none)."""
    cum, cumrel, nbits = _tables(cum, cumrel)
    count, total, tsum = cumrel[:, 1:nbits + 2], cum[:, 1:nbits + 2], cumrel[:, nbits + 1:nbits + 2]
    live = tsum > 0
    zero = torch.zeros_like(count)
    p = torch.where(live, count / torch.where(total == 0, torch.full_like(total, 0.1), total), zero)
    r = torch.where(live, count / tsum.clamp(min=1), zero)
    mask = (p > 0).double().sum(0)
    mask = torch.where(mask == 0, torch.full_like(mask, 0.1), mask)
    return p.sum(0) / mask, r.sum(0) / mask


def precision_within_radius(cum, cumrel, radius=2):
    """Mean over ALL queries of (relevant rows within `radius`) / (rows within `radius`), 0 for a query that finds nothing:
    get_precision_recall_by_Hamming_Radius (:577-594), P@H<=2 at the default."""
    cum, cumrel, nbits = _tables(cum, cumrel)
    if cum.shape[0] == 0:
        raise ZeroDivisionError("precision_within_radius: no queries")
    b = min(int(radius // 1), nbits) + 1                  # distances are integers: d <= radius <=> d < floor(radius) + 1
    if b < 1:
        return 0.0
    found, hit = cum[:, b], cumrel[:, b]
    return torch.where(found > 0, hit / found.clamp(min=1), torch.zeros_like(hit)).mean().item()


def _radius_tables(query_codes, database_codes, query_labels, database_labels, device, what):
    """+-1 codes and multi-hot labels -> (cum, cumrel): packed, prepared and counted on the GPU, or with an explicit
    device='cpu' through the host twins.  Nothing the caller passed is modified."""
    B = backend(device)
    Hm = B.H
    q, r, ql, rl = (B.move(t) for t in (query_codes, database_codes, query_labels, database_labels))
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1] or ql.dim() != 2 or rl.dim() != 2 or ql.shape[1] != rl.shape[1]:
        raise ValueError(f"{what}: expected [Q, nbits] / [N, nbits] codes and [Q, classes] / [N, classes] multi-hot labels")
    nbits = q.shape[1]
    if nbits > 128 or rl.shape[1] > 128:
        raise ValueError(f"{what}: +-1 codes of at most 128 bits and at most 128 classes (got {nbits} bits, {rl.shape[1]} classes)")
    qp, rp = Hm.pack_codes(q), Hm.pack_codes(r)           # raises ValueError for anything but exactly +1 / -1
    qlp, rlp = Hm.pack_labels(ql), Hm.pack_labels(rl)
    got = Hm.hamming_radius_hist(qp, Hm.PreparedDB(rp, nbits), Hm.PreparedLabels(rlp), qlp, nbits)
    if got is None:
        raise ValueError(f"{what}: {r.shape[0]} rows are outside the radius histograms (at most {64 * SHARD_ROWS_MAX} on the GPU)")
    return got


def pr_curve(qB, rB, query_label, retrieval_label, device=None):
    """The reference's pr_curve (:469-493), same name and argument order -> (P, R) float64 [nbits + 1]."""
    return radius_curves(*_radius_tables(qB, rB, query_label, retrieval_label, device, "pr_curve"))


def get_precision_recall_by_Hamming_Radius(database_output, database_labels, query_output, query_labels, radius=2, device=None):
    """The reference's function of this name (:577-594), same argument order -> float.  Unlike the reference it leaves
    `query_labels` as it was (the reference overwrites its zeros with -1)."""
    tables = _radius_tables(query_output, database_output, query_labels, database_labels, device, "get_precision_recall_by_Hamming_Radius")
    return precision_within_radius(*tables, radius=radius)
