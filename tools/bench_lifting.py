"""The batched tensor tail (ToTensor -> Normalize -> CustomTransform as ONE call, wv_lift_images) against the best batched
composition the code offered before it, in ONE run, on sized uint8 NHWC batches (what size_images returns):

    python tools/bench_lifting.py [--out profiles/lifting_batched.json] [--batch 2048] [--rounds 7] [--calls 3]

Cases: haar, one level, 224 x 224 (cub_dwt); haar, three levels, 224 x 224; cdf 9/7, one level, 448 x 448 (cub_dwt_cdf97,
batch / 4 images: the same number of pixels).  Per case, timed in the same alternating rounds with HIP events:
  a  lift_images(x, mean, std, ...): the new call, output allocation included
  b  the composition as the code ran it before wv_lift_images existed: torch permute / float().div(255) / sub / div, then
     the level cascade of HaarLifting / Cdf97Lifting on the GPU tensor = per level F.pad, wv_lifting2d_forward (two launches
     through a plane-sized scratch), and torch.cat of the bands (CustomTransform is not used: it is one wv_lift_images call)
  c  a device-to-device copy of as many bytes as a's algorithmic bytes (the uint8 batch read once + the fp32 result written
     once).  A copy reads AND writes each of them, so c moves TWICE the traffic a must move: a call that moved its bytes
     at the copy's rate would show a_over_c = 0.5, and a_over_c = 1 is half that rate.  c_moved_bytes_per_s is the copy's
     own rate (read + write), to set beside a's bytes_per_s
Prints one JSON row: per case ms medians, images / s of a, algorithmic bytes / s of a, a_over_b and a_over_c (time ratios:
below 1 = a is faster), `equal` (a's bits = the bits of the old lifting path fed by ToTensor / Normalize run on the HOST, as the
workers run them; first 64 images, checked before anything is timed) and `b_max_abs_diff` (a against b as timed: torch's GPU
division by a scalar multiplies by the reciprocal, so b is not the workers' `.div(255)` to the last bit).
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash.transforms import Cdf97Lifting, HaarLifting, lift_images  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = (("haar_l1_224", "haar", 1, 224, 1), ("haar_l3_224", "haar", 3, 224, 1), ("cdf97_l1_448", "cdf97", 1, 448, 4))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def cascade(basis, levels):
    dwt = (HaarLifting if basis == "haar" else Cdf97Lifting)(n_levels=levels)

    def run(t):
        approx, details = dwt(t)
        return torch.cat([approx[-1].unsqueeze(-3), details[-1]], dim=-3)
    return run


def composition(x, basis, levels):
    m = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    ct = cascade(basis, levels)

    def run():
        return ct(x.permute(0, 3, 1, 2).float().div(255).sub(m).div(s))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lifting: needs the GPU (a rate measured elsewhere says nothing about it)")
    row = {"what": "wv_lift_images (a) vs torch ops + wv_lifting2d_forward per level + cat, as the code ran before it (b) vs "
                   "a device-to-device copy of the algorithmic bytes (c); uint8 NHWC in, ImageNet Normalize",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls": args.calls, "cases": {}}
    for name, basis, levels, side, div in CASES:
        B = max(1, args.batch // div)
        x = torch.from_numpy(np.random.default_rng(side + levels).integers(0, 256, (B, side, side, 3), dtype=np.uint8)).cuda()
        fa = lambda: lift_images(x, MEAN, STD, basis=basis, levels=levels, channels_last=True)      # noqa: E731
        fb = composition(x, basis, levels)
        ya, yb = fa(), fb()
        # torch's GPU kernels divide by a scalar as a multiplication with its reciprocal, so b as timed is not ToTensor's
        # .div(255) of the workers to the last bit: `equal` compares a with the old lifting path fed by the HOST conversion
        n = min(B, 64)
        m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
        host = x[:n].cpu().permute(0, 3, 1, 2).float().div(255).sub_(m).div_(s)
        yh = cascade(basis, levels)(host.cuda())
        equal = bool(torch.equal(ya[:n].view(torch.int32), yh.contiguous().view(torch.int32)))
        b_max_abs_diff = float((ya - yb).abs().max())
        nbytes = x.numel() + ya.numel() * 4
        del yb, yh
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        fc = lambda: dst.copy_(src)                                                                # noqa: E731
        for _ in range(5):                                                                         # clock warm-up
            fa(), fb(), fc()
        ta, tb, tc = [], [], []
        for _ in range(args.rounds):                                                               # alternating
            ta.append(timed(fa, args.calls))
            tb.append(timed(fb, args.calls))
            tc.append(timed(fc, args.calls))
        a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
        row["cases"][name] = {"batch": B, "side": side, "basis": basis, "levels": levels, "equal": equal, "b_max_abs_diff": b_max_abs_diff,
                              "a_ms_median": round(a, 4), "a_ms_min": round(min(ta), 4), "a_ms_max": round(max(ta), 4),
                              "b_ms_median": round(b, 4), "c_ms_median": round(c, 4), "images_per_s": round(B / a * 1e3, 1),
                              "algorithmic_bytes": nbytes, "bytes_per_s": round(nbytes / a * 1e3, 1),
                              "c_copied_bytes": nbytes, "c_moved_bytes": 2 * nbytes, "c_moved_bytes_per_s": round(2 * nbytes / c * 1e3, 1),
                              "a_over_b": round(a / b, 4), "a_over_c": round(a / c, 4)}
        del x, ya, src, dst
        torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
