#!/usr/bin/env python3
"""Where each role of the sliding SWT kernel spends its cycles (diagnostic build: tools/build_variant.sh swtstamps swt_slide.hip
-DWV_SWT_STAMPS, run with WVHASH_LIB=tools/_variants/swtstamps.so).  One warm and one measured launch of db2 level 3 on 2048
planar uint8 images of 224 x 224; cycles per segment of a chunk, summed over the launch, averaged over the waves of the role."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-retrieval-wavelet_amd"))
import torch  # noqa: E402

from wvhash import _lib  # noqa: E402
from wvhash.transforms import swt2d  # noqa: E402


def main():
    fn = _lib.load().wv_debug_swt_stamps
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    buf = (ctypes.c_ulonglong * 16)()
    img = torch.randint(0, 256, (2048, 3, 224, 224), dtype=torch.uint8, device="cuda")
    out = torch.empty((2048, 3, 4, 224, 224), dtype=torch.float32, device="cuda")
    for _ in range(2):                       # the first launch warms up; reading clears the sums
        swt2d(img, "db2", 3, out=out)
        torch.cuda.synchronize()
        if fn(buf, 16):
            raise SystemExit("wv_debug_swt_stamps failed")
    v, h = list(buf[0:8]), list(buf[8:16])   # [role][segment]
    # waves per role: 4 in each workgroup of the persistent grid (slide_launch: two workgroups per CU, a multiple of 8)
    grid = min(2048 * 3, 2 * torch.cuda.get_device_properties(0).multi_processor_count)
    nv = nh = 4 * (grid - grid % 8 if grid < 2048 * 3 else grid)
    print(f"[swt stamps] V waves={nv}: LDS read+lower(pl0) {v[0] / nv:.0f} | rest(last+stores, pl1) {v[1] / nv:.0f} | "
          f"barrier {v[2] / nv:.0f}")
    print(f"[swt stamps] H waves={nh}: wait loads+convert {h[0] / nh:.0f} | issue next loads {h[1] / nh:.0f} | "
          f"lower levels {h[2] / nh:.0f} | last level+LDS write {h[3] / nh:.0f} | barrier {h[4] / nh:.0f}")


if __name__ == "__main__":
    main()
