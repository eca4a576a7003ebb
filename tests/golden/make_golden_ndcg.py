#!/usr/bin/env python3
"""Regenerates tests/golden/ndcg_golden.npz:   python tests/golden/make_golden_ndcg.py <root of the reference checkout>

The file pins NDCG and precision at top-K against the REFERENCE's own code.  cos, hamming, euclidean, NDCG, calc_hamming_dist
and p_topK (main/engine/DSCH/_utils.py:453-466, 496-574) need only numpy and torch; their FunctionDef nodes are cut out of
the reference file with `ast` at generation time (the `_cut` pattern of make_golden_radius.py -- nothing of the source is
stored), compiled unmodified and run on seeded cases.  The namespace's `np` is a proxy that records what np.argsort returned
(as make_golden.py does for torch.argsort): the order the reference's unstable sort produced is stored with the value it led
to.  Stored: inputs (codes as packed bits, labels as uint8, real features as float32; the six cases shared with
radius_golden.npz are asserted equal to that file's inputs and read from there, not stored twice), the recorded orders as int32 (their first
250 columns: the size limit), the reference's NDCG at k in {1, 7, 50, N / 2, -1} and its
p_topK at K = [1, 5, 50, N].  Data only.  No test reads the reference; tests read the .npz.

Cases: the six of make_golden_radius.py (same make_case: lone queries, planted rows at distance 0, two label words; largest
overlap 3), a dense-label case (20 classes, overlap up to 20), a two-word case whose overlaps span both label words, and two
real-valued tie-free cases (cosine, squared L2) whose neighbouring scores are at least 1e-4 apart, so that fp32 and fp64
rank alike.  Every stored reference value is asserted to lie inside the interval tie-breaking can produce.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import ndcg_cases as C                                      # noqa: E402
from make_golden_radius import CASES as RADIUS_CASES, _cut, make_case, pack_bits   # noqa: E402

MIN_GAP = 1e-4
ORDER_COLS = 250            # columns of the recorded orders that are stored (the size limit)


class _RecordingNumpy(object):
    """numpy, except that argsort's results are kept."""

    def __init__(self):
        self.orders = []

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, *args, **kwargs):
        out = np.argsort(*args, **kwargs)
        self.orders.append(out)
        return out


def load_reference(ref_root):
    funcs = _cut(os.path.join(ref_root, "main", "engine", "DSCH", "_utils.py"),
                 ["calc_hamming_dist", "p_topK", "cos", "hamming", "euclidean", "NDCG"])
    import ast
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    rec = _RecordingNumpy()
    ns = {"torch": torch, "np": rec}
    exec(compile(mod, "<reference DSCH/_utils.py (cut)>", "exec"), ns)
    return ns["NDCG"], ns["p_topK"], rec


def clustered_codes(lab, nbits, g, flip=0.12):
    centres = torch.randint(0, 2, (lab.shape[1], nbits), generator=g).float() * 2 - 1
    sign = (torch.rand(lab.shape[0], nbits, generator=g) < flip).float() * -2 + 1
    return centres[lab.argmax(1)] * sign


def dense_case(seed):
    """20 classes at p = 0.4: overlaps up to 20.  Query 0 and row 0 carry every class, row 1 none."""
    g = torch.Generator().manual_seed(seed)
    Q, N, nbits, classes = 8, 120, 32, 20
    ql = (torch.rand(Q, classes, generator=g) < 0.4).float()
    rl = (torch.rand(N, classes, generator=g) < 0.4).float()
    ql[0], rl[0], rl[1] = 1, 1, 0
    ql[ql.sum(1) == 0, 0] = 1
    return clustered_codes(ql, nbits, g), clustered_codes(rl, nbits, g), ql, rl


def two_word_case(seed):
    """100 classes at p = 0.1; query 3 and row 7 share seven classes, of both label words."""
    g = torch.Generator().manual_seed(seed)
    Q, N, nbits, classes = 10, 150, 48, 100
    ql = (torch.rand(Q, classes, generator=g) < 0.1).float()
    rl = (torch.rand(N, classes, generator=g) < 0.1).float()
    for c in (3, 10, 20, 70, 80, 90, 95):
        ql[3, c] = rl[7, c] = 1
    ql[ql.sum(1) == 0, 0] = 1
    rl[rl.sum(1) == 0, 1] = 1
    return clustered_codes(ql, nbits, g), clustered_codes(rl, nbits, g), ql, rl


def real_case(what, seed, Q=12, N=200, D=24, classes=10):
    """float32 features chosen so that, for every query, neighbouring ranking keys are >= MIN_GAP apart (candidates that
    would come closer to an accepted row are dropped)."""
    g = torch.Generator().manual_seed(seed)
    grid = lambda t: torch.round(t * 32) / 32                # multiples of 1/32: exact in fp32, and the file stays small
    q = grid(torch.randn(Q, D, generator=g))
    ql = (torch.rand(Q, classes, generator=g) < 0.25).float()
    ql[0] = 0
    rows, keys = [], np.zeros((Q, 0))
    while len(rows) < N:
        cand = grid(torch.randn(1, D, generator=g))
        key = C.scores_np({"q": q, "r": cand, "what": what})                 # [Q, 1]
        if keys.shape[1] == 0 or np.abs(keys - key).min() >= 1.5 * MIN_GAP:
            rows.append(cand)
            keys = np.concatenate([keys, key], axis=1)
    r = torch.cat(rows)
    rl = (torch.rand(N, classes, generator=g) < 0.25).float()
    gap = np.diff(np.sort(C.scores_np({"q": q, "r": r, "what": what}), axis=1), axis=1).min()
    assert gap >= MIN_GAP, gap
    return q, r, ql, rl


def main(ref_root):
    ref_ndcg, ref_ptopk, rec = load_reference(ref_root)
    cases = [(name, 1, make_case(Q, N, nbits, classes, planted, 1000 + ci))
             for ci, (name, Q, N, nbits, classes, planted) in enumerate(RADIUS_CASES)]
    cases += [("dense_q8_n120_k20", 1, dense_case(2001)), ("two_q10_n150_k100", 1, two_word_case(2002)),
              ("cos_q12_n200_d24", 0, real_case(0, 2003)), ("l2_q12_n200_d24", 2, real_case(2, 2004))]
    assert [c[0] for c in cases] == C.HAMMING_CASES + C.REAL_CASES
    out = {}
    for name, what, (q, r, ql, rl) in cases:
        Q, N = q.shape[0], r.shape[0]
        qn, rn, qln, rln = (t.double().numpy() for t in (q, r, ql, rl))
        Rel = C.overlaps(qln, rln)
        assert Rel.max() <= 52, (name, Rel.max())              # the reference's int64 gains are exact
        if name.startswith("dense"):
            assert Rel.max() == 20 and (Rel[:, 1] == 0).all()
        if name.startswith("two"):
            w0, w1 = C.overlaps(qln[:, :64], rln[:, :64]), C.overlaps(qln[:, 64:], rln[:, 64:])
            assert Rel.max() >= 6 and ((w0 > 0) & (w1 > 0) & (Rel >= 6)).any(), name
        case = {"q": q, "r": r, "what": what}
        d = C.scores_np(case)
        ks, vals, order = C.ndcg_ks(N), [], None
        for k in ks:
            del rec.orders[:]
            vals.append(float(ref_ndcg(qn.copy(), rn.copy(), qln.copy(), rln.copy(), what=what, k=k)))
            assert len(rec.orders) == 1 and (order is None or np.array_equal(order, rec.orders[0]))
            order = rec.orders[0]
            kk = N if k < 0 else k
            lo, hi = C.ndcg_tie_bounds(d, Rel, kk)
            assert lo - C.ndcg_tol(kk) <= vals[-1] <= hi + C.ndcg_tol(kk), (name, k, lo, vals[-1], hi)
            assert abs(C.ndcg_restated(order, Rel, kk) - vals[-1]) <= C.ndcg_tol(kk), (name, k)
        cols = min(N, ORDER_COLS)
        out.update({f"{name}/ql": ql.numpy().astype(np.uint8), f"{name}/rl": rl.numpy().astype(np.uint8),
                    f"{name}/what": np.array([what]), f"{name}/order": order[:, :cols].astype(np.int32),
                    f"{name}/ks": np.array(ks), f"{name}/ref_ndcg": np.array(vals, dtype=np.float64)})
        msg = f"{name}: max overlap {Rel.max()}, NDCG@{ks} = {[round(v, 6) for v in vals]}"
        shared = name in C.SHARED_WITH_RADIUS
        if shared:                                             # same make_case, same seed: the inputs are already committed
            import radius_cases
            have = radius_cases.load_golden(HERE, name)
            assert all(torch.equal(have[key], t) for key, t in (("q", q), ("r", r), ("ql", ql), ("rl", rl))), name
            del out[f"{name}/ql"], out[f"{name}/rl"]
        if what == 1:
            K = [N if x is None else x for x in C.P_TOPK_K]
            p = ref_ptopk(q.clone(), r.clone(), ql.clone(), rl.clone(), K=list(K)).numpy()
            lo, hi = C.ptopk_tie_bounds(d, Rel > 0, K)
            assert (lo - C.ptopk_tol(Q) <= p).all() and (p <= hi + C.ptopk_tol(Q)).all(), (name, lo, p, hi)
            if not shared:
                out.update({f"{name}/q": pack_bits(q), f"{name}/r": pack_bits(r), f"{name}/nbits": np.array([q.shape[1]])})
            out.update({f"{name}/K": np.array(K), f"{name}/ref_ptopk": p})
            msg += f"   p_topK@{K} = {[round(float(v), 5) for v in p]}"
        else:
            out.update({f"{name}/q": q.numpy().astype(np.float32), f"{name}/r": r.numpy().astype(np.float32)})
        print(msg)
    path = os.path.join(HERE, "ndcg_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    main(sys.argv[1])
