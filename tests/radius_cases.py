"""Shared by tests/test_host_radius_hist.py and tests/test_gpu_radius_hist.py: the brute-force expectation of the radius
histograms (torch, from the +-1 codes and multi-hot labels), seeded inputs with the edge cases planted, and the
reference-made fixture tests/golden/radius_golden.npz (made by tests/golden/make_golden_radius.py; data only)."""
import os

import numpy as np
import torch

GOLDEN_CASES = ["c16_q9_n70_k5", "c32_q16_n300_k12", "c48_q24_n500_k38", "c64_q32_n1000_k38", "c128_q40_n777_k80", "far_q9_n70_k5"]


def golden_tol(Q):
    """Absolute tolerance against the reference-made values: the reference divides once in fp32 per query and sums Q
    values <= 1 in fp32; ours is float64 from exact integers."""
    return (Q + 3) * 2.0 ** -24


def brute_tables(q, r, ql, rl, chunk=64):
    """+-1 codes q [Q, nbits], r [N, nbits], multi-hot labels -> (cum, cumrel) int32 [Q, nbits + 2] on q's device:
    d = (nbits - q @ r.T) / 2 (exact in fp32 for nbits <= 128), rel = ql @ rl.T > 0, scatter_add, exclusive cumulative sum."""
    Q, nbits = q.shape
    cnt = torch.zeros((2, Q, nbits + 2), dtype=torch.int64, device=q.device)
    r, rl = r.float(), rl.float()
    for s in range(0, Q, chunk):                           # [chunk, N] temporaries only
        d = ((nbits - q[s:s + chunk].float() @ r.t()) / 2).long()
        rel = (ql[s:s + chunk].float() @ rl.t() > 0).long()
        cnt[0, s:s + chunk].scatter_add_(1, d + 1, torch.ones_like(d))
        cnt[1, s:s + chunk].scatter_add_(1, d + 1, rel)
    cum = cnt.cumsum(2)                                    # counts of bin d sit at [d + 1]: cum[b] = rows with distance < b
    return cum[0].int(), cum[1].int()


def make_inputs(Q, N, nbits, classes, seed, identical=False):
    """Seeded +-1 codes and multi-hot labels with the cases a radius histogram can get wrong planted in:
    query 0 has no class (zero label words); with two label words and Q > 1 the last query has classes of the SECOND word
    only (and some rows carry them); rows 0.. duplicate query codes (distance 0), relevant and not; clustered codes (few bins, ties).
    identical: every row has the same code (every row in one bin: the cell-overflow case)."""
    g = torch.Generator().manual_seed(seed)
    p = min(0.5, 2.0 / classes)
    ql = (torch.rand(Q, classes, generator=g) < p).float()
    rl = (torch.rand(N, classes, generator=g) < p).float()
    ql[ql.sum(1) == 0, 1] = 1.0
    ql[0] = 0
    if classes > 64 and Q > 1:                             # a single query stays the lone one
        ql[Q - 1] = 0
        ql[Q - 1, 64 + (seed % (classes - 64))] = 1.0
        ql[Q - 1, classes - 1] = 1.0
    centres = torch.randint(0, 2, (8, nbits), generator=g).float() * 2 - 1
    flip = lambda n: (torch.rand(n, nbits, generator=g) < 0.1).float() * -2 + 1
    q = centres[torch.randint(0, 8, (Q,), generator=g)] * flip(Q)
    if identical:
        r = q[Q // 2].repeat(N, 1)
    else:
        r = centres[torch.randint(0, 8, (N,), generator=g)] * flip(N)
        for i in range(min(Q, N // 2, 4)):                 # duplicates of query codes: rows 2i (relevant unless the query is
            r[2 * i] = q[i]                                # lone) and 2i + 1 (not relevant)
            r[2 * i + 1] = q[i]
            rl[2 * i] = ql[i]
            rl[2 * i + 1] = 0
            rl[2 * i + 1, int((ql[i] == 0).nonzero()[0])] = 1.0
    return q, r, ql, rl


def load_golden(golden_dir, name):
    """-> dict: q, r (+-1 float), ql, rl (float 0/1), nbits, ref_P, ref_R (float32), radii, ref_prec (float64)."""
    z = np.load(os.path.join(golden_dir, "radius_golden.npz"))
    nbits = int(z[f"{name}/nbits"][0])
    unpack = lambda a: torch.from_numpy(np.unpackbits(a, axis=1)[:, :nbits].astype(np.float32)) * 2 - 1
    return {"q": unpack(z[f"{name}/q"]), "r": unpack(z[f"{name}/r"]), "nbits": nbits,
            "ql": torch.from_numpy(z[f"{name}/ql"]).float(), "rl": torch.from_numpy(z[f"{name}/rl"]).float(),
            "ref_P": z[f"{name}/ref_P"].astype(np.float64), "ref_R": z[f"{name}/ref_R"].astype(np.float64),
            "radii": [int(x) for x in z[f"{name}/radii"]], "ref_prec": z[f"{name}/ref_prec"]}
