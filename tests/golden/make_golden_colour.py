#!/usr/bin/env python3
"""Regenerates tests/golden/colour_golden.npz:   python tests/golden/make_golden_colour.py

The file pins the colour jitter against Pillow's ImageEnhance AS OF THE VERSION THAT WROTE IT (stored in the file: 12.2.0).
tests/test_host_colour.py compares the library with the live Pillow on many more cases; this handful of stored inputs and
outputs tells the two possible failures apart: when the live Pillow no longer reproduces the stored outputs, Pillow changed
-- not the library.  Data only: small uint8 images, the chain of each (kinds, fp32 factors) and Pillow's output.
"""
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import colour_cases as C   # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    cases = C.golden_cases()
    out["n"] = np.array(len(cases))
    for i, (arr, chain) in enumerate(cases):
        out[f"in_{i}"] = arr
        out[f"kind_{i}"] = np.array([k for k, _ in chain], np.int32)
        out[f"factor_{i}"] = np.array([f for _, f in chain], np.float32)
        out[f"out_{i}"] = C.pillow_chain(arr, chain)
    path = os.path.join(HERE, "colour_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
