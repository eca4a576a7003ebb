#!/usr/bin/env python3
"""Regenerates tests/golden/swt_anchor_golden.npz.  Run in the BUILD container only (needs /root/reference):
    python tests/golden/make_golden_swt_anchor.py

The reference's Daubechies-4 (= db2) lifting, /root/reference/main/transforms/wavelets/daub_4.py, run level after level on
LL the way CustomTransform cascades HaarLifting / Cdf97Lifting (custom_transforms.py:26-33): the outside anchor of the
db2 SWT / DWT restatement (tests/swt_anchor_cases.py).  The module is imported by file path through the loader of
make_golden_lifting.py; the lifting kernel, the two scale flags and the 2-D scales are read from the reference's
modules at run time, nothing of them is written down here.  `fast_daub4_2d_op` returns the four bands merged into the
channel axis; the reference's own `extract_coeffs_from_channels` takes them apart again.
Fixtures are data only: inputs (as seeds + shapes) and expected outputs, keyed like lifting_golden.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden_lifting import load_reference_wavelets  # noqa: E402

CASES = [  # name, shape [N,C,H,W], levels, seed
    ("db2_224", (1, 1, 224, 224), 3, 9),
    ("db2_64x96", (1, 2, 64, 96), 2, 10),                    # non-square, two planes
    ("db2_40x30", (1, 2, 40, 30), 1, 11),                    # W % 4 != 0: the generic SWT kernels
]


def main():
    _, _, daub, utils = load_reference_wavelets(daub4=True)
    out = {}
    for name, shape, levels, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        cur = torch.randn(shape, generator=g)
        out[f"{name}/seed"] = np.array(seed)
        out[f"{name}/shape"] = np.array(shape)
        for lev in range(levels):
            assert cur.shape[-2] % 2 == 0 and cur.shape[-1] % 2 == 0
            y = daub.fast_daub4_2d_op(cur.clone(), daub.DEFAULT_KERNEL, utils.DEFAULT_SCALE_1D_COEFFS,
                                      utils.DEFAULT_SCALE_2d_COEFFS, utils.COEFFS_SCALES_2D)
            ll, lh, hl, hh = utils.extract_coeffs_from_channels(y)
            assert ll.dtype == torch.float32
            out[f"{name}/l{lev}/ll"] = ll.numpy().copy()
            out[f"{name}/l{lev}/hi"] = torch.stack([lh, hl, hh], dim=-3).numpy().copy()
            cur = ll.clone()
    path = os.path.join(HERE, "swt_anchor_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
