#!/usr/bin/env python3
"""Regenerates tests/golden/image_size_golden.npz:   python tests/golden/make_golden_image_size.py

The file pins the image sizing against Pillow's 8-bit resampler AS OF THE VERSION THAT WROTE IT (stored in the file:
12.2.0).  tests/test_host_image_size.py compares the library with the live Pillow on many more cases; this handful of
stored inputs and outputs tells the two possible failures apart: when the live Pillow no longer reproduces the stored
outputs, Pillow changed -- not the library.  Data only: seeded uint8 images, the stage of each and Pillow's output.
"""
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import image_size_cases as C   # noqa: E402


def golden_cases():
    """A handful of the tests' cases, each below 64 x 64 x 3 bytes in and out."""
    cases = []
    for i in (0, 1, 6, 9, 10, 11):
        w, h, ow, oh = C.FIXED_PAIRS[i]
        arr = C.image(w, h, "noise" if i % 2 == 0 else "binary", 100 + i)
        for f in (C.BILINEAR, C.BICUBIC):
            cases.append((arr, C.stage(arr, (ow, oh), f)))
    a = C.image(61, 45, "noise", 1)
    cases.append((a, C.stage(a, (20, 17), C.BILINEAR, crop=(7, 5, 40, 33))))
    cases.append((a, C.stage(a, (30, 22), C.BICUBIC, window=(4, 2, 20, 40), flip=1)))
    cases.append((a, C.stage(a, (30, 22), C.BILINEAR, window=(-5, -3, 44, 30))))
    return cases


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    cases = golden_cases()
    out["n"] = np.array(len(cases))
    for i, (arr, st) in enumerate(cases):
        out[f"in_{i}"] = arr
        out[f"stage_{i}"] = np.array(list(st["crop"]) + list(st["res"]) + list(st["win"]) + [st["filter"], st["flip"]], np.int32)
        out[f"out_{i}"] = C.pillow_stage(arr, st)
    path = os.path.join(HERE, "image_size_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
