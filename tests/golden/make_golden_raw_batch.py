#!/usr/bin/env python3
"""RUN AT THE PARENT of the change that made sizing.py's two descriptor tables share one record path (the commit before
"Image pipeline: one record path ..."), never with the code it pins:   python tests/golden/make_golden_raw_batch.py

Writes tests/golden/raw_batch_golden.npz: what ``sizing.raw_collate`` packed THEN for the three batches of
``colour_cases.raw_batches()`` -- ``data`` (its SHA-256 where the bytes would be large), ``desc``, ``colour``, ``launches``,
``colour_launches``, ``out_shape`` and ``work_bytes``.  tests/test_host_image_size.py rebuilds the batches with the live
code and compares every array and tuple for equality.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "image-retrieval-wavelet_amd"))
sys.path.insert(0, os.path.dirname(HERE))

import colour_cases as C   # noqa: E402


def main():
    batches = C.raw_batches()
    path = os.path.join(HERE, "raw_batch_golden.npz")
    np.savez_compressed(path, **C.raw_batch_arrays(batches))
    for name, rb in batches.items():
        print(name, rb.launches, rb.colour_launches, rb.out_shape, rb.work_bytes)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
