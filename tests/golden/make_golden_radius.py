#!/usr/bin/env python3
"""Regenerates tests/golden/radius_golden.npz:   python tests/golden/make_golden_radius.py <root of the reference checkout>

The file pins precision / recall by Hamming radius against the REFERENCE's own code.  calc_hamming_dist, pr_curve and
get_precision_recall_by_Hamming_Radius (main/engine/DSCH/_utils.py:453-493, 577-594) need only torch and numpy; their
FunctionDef nodes are cut out of the reference file with `ast` at generation time (the `_cut` pattern of make_golden.py --
nothing of the source is stored), compiled unmodified and run on seeded cases.  Stored: inputs (codes as packed bits, labels
as uint8) and the reference's outputs.  Data only.  No test reads the reference; tests read the .npz.

Every table case holds: lone queries (no class at all, or a class no row carries), database rows EQUAL to a query code
(distance 0) that are relevant and that are not, and radii within which some query finds nothing.  A row equal to a query
code rules out a radius at which NO query finds anything, so that situation -- the 0.1 stand-ins of pr_curve for "found
nothing" and "no query with a hit" -- has a small-N case of its own without planted rows (`far_*`).
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # name, Q, N, nbits, classes, planted rows
    ("c16_q9_n70_k5", 9, 70, 16, 5, True),
    ("c32_q16_n300_k12", 16, 300, 32, 12, True),
    ("c48_q24_n500_k38", 24, 500, 48, 38, True),
    ("c64_q32_n1000_k38", 32, 1000, 64, 38, True),
    ("c128_q40_n777_k80", 40, 777, 128, 80, True),        # two label words
    ("far_q9_n70_k5", 9, 70, 64, 5, False),               # random 64-bit codes: nothing within small radii for any query
]
FLIP = 0.12


def _cut(path, names):
    with open(path, "r") as f:
        tree = ast.parse(f.read(), filename=path)
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    missing = [n for n in names if n not in found]
    if missing:
        raise RuntimeError(f"{path}: {missing} not found")
    return [found[n] for n in names]


def load_reference(ref_root):
    funcs = _cut(os.path.join(ref_root, "main", "engine", "DSCH", "_utils.py"),
                 ["calc_hamming_dist", "pr_curve", "get_precision_recall_by_Hamming_Radius"])
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "np": np}
    exec(compile(mod, "<reference DSCH/_utils.py (cut)>", "exec"), ns)
    return ns["pr_curve"], ns["get_precision_recall_by_Hamming_Radius"]


def make_case(Q, N, nbits, classes, planted, seed):
    g = torch.Generator().manual_seed(seed)
    p = min(0.5, 1.6 / classes)

    def labels(n):
        lab = (torch.rand(n, classes, generator=g) < p).float()
        empty = lab.sum(1) == 0
        lab[empty, torch.randint(0, classes - 1, (n,), generator=g)[empty]] = 1.0
        return lab

    ql, rl = labels(Q), labels(N)
    for lab in (ql, rl):                                   # the last class: no row carries it, and one lone query only
        lab[:, classes - 1] = 0
        lab[lab.sum(1) == 0, 0] = 1.0
    ql[0] = 0                                              # lone: no class at all
    ql[1] = 0
    ql[1, classes - 1] = 1.0                               # lone: only the class no row carries
    if classes > 64:
        ql[2] = 0
        ql[2, 70] = 1.0                                    # only classes of the second label word
        rl[5, 70] = 1.0
    if not planted:
        q = torch.randint(0, 2, (Q, nbits), generator=g).float() * 2 - 1
        r = torch.randint(0, 2, (N, nbits), generator=g).float() * 2 - 1
        return q, r, ql, rl
    centres = torch.randint(0, 2, (classes, nbits), generator=g).float() * 2 - 1

    def codes(lab):
        first = lab.argmax(1)                              # centre of the row's first class, 12 % of the bits flipped
        flip = (torch.rand(lab.shape[0], nbits, generator=g) < FLIP).float() * -2 + 1
        return centres[first] * flip

    q, r = codes(ql), codes(rl)
    # rows equal to a query code: relevant (the query's labels) and not relevant (a class the query lacks)
    for i, (qi, row) in enumerate([(3, 10), (4, 11), (5, 12)]):
        r[row] = q[qi]
        rl[row] = ql[qi]
        r[row + 10] = q[qi]
        rl[row + 10] = 0
        rl[row + 10, int((ql[qi] == 0).nonzero()[0])] = 1.0
    r[40] = q[0]                                           # equal to a lone query's code
    return q, r, ql, rl


def pack_bits(codes):
    return np.packbits((codes.numpy() > 0).astype(np.uint8), axis=1)


def main(ref_root):
    ref_pr_curve, ref_radius = load_reference(ref_root)
    out, mixed = {}, 0
    for ci, (name, Q, N, nbits, classes, planted) in enumerate(CASES):
        q, r, ql, rl = make_case(Q, N, nbits, classes, planted, 1000 + ci)
        P, R = ref_pr_curve(q.clone(), r.clone(), ql.clone(), rl.clone())
        radii = [0, 2, nbits // 4]
        prec = [float(ref_radius(r.numpy().copy(), rl.numpy().copy(), q.numpy().copy(), ql.numpy().copy(), radius=rad))
                for rad in radii]                          # copies: the reference overwrites its label argument
        d = (nbits - q @ r.t()) / 2
        found = torch.stack([(d <= rad).sum(1) for rad in range(nbits + 1)], 1)
        assert bool((ql.sum(1) == 0).any()) and bool(((ql @ rl.t()) > 0).sum(1).eq(0).sum() >= 2), name
        assert bool((found == 0).any()), name               # some query finds nothing within some radius
        if planted:
            rel = (ql @ rl.t()) > 0
            assert bool(((d == 0) & rel).any()) and bool(((d == 0) & ~rel).any()), name
        else:
            assert bool((found == 0).all(0).any()), name    # radii at which no query finds anything
        mixed += 0.0 < prec[1] < 1.0
        out.update({f"{name}/q": pack_bits(q), f"{name}/r": pack_bits(r), f"{name}/ql": ql.numpy().astype(np.uint8),
                    f"{name}/rl": rl.numpy().astype(np.uint8), f"{name}/nbits": np.array([nbits]),
                    f"{name}/ref_P": P.numpy(), f"{name}/ref_R": R.numpy(),
                    f"{name}/radii": np.array(radii), f"{name}/ref_prec": np.array(prec, dtype=np.float64)})
        print(f"{name}: P@H<=0/2/{nbits // 4} = {prec[0]:.4f} / {prec[1]:.4f} / {prec[2]:.4f}   P[0..3] {P[:4].tolist()}")
    assert mixed >= 3, f"P@H<=2 is strictly between 0 and 1 in only {mixed} cases"
    path = os.path.join(HERE, "radius_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    main(sys.argv[1])
