"""Colour jitter on the GPU against Pillow on the host, in ONE run: B = 2048 images of 500 x 375 through the VOC train node
(Resize(256) -> RandomResizedCrop(224) -> ColorJitter(0.25, 0.25, 0.25, hue 0) -> RandomHorizontalFlip), the jitter on the
224 x 224 images the sizing wrote.

    python tools/bench_colour.py [--out profiles/colour_jitter.json] [--batch 2048] [--rounds 7] [--calls 5] [--procs 16]

Prints one JSON row:
  images_per_s         wv_colour_jitter alone (descriptors and sized images resident on the device; the workspace clear and both
                       launches), HIP events, median of the rounds.  The call works in place, so every timed call jitters what
                       the one before left; the kernels have no data-dependent path
  bytes_per_s          algorithmic bytes over that time: the image read by the statistics launch, read again and written by the
                       apply launch, 3 * 224 * 224 * 3 = 451,584 bytes per image (every image of this node has contrast)
  copy_fraction        that rate over the rate of a device-to-device copy of the same number of bytes, timed in the same
                       rounds (a copy moves its bytes twice: read + write)
  pillow_images_per_s  ColorJitter on PIL images alone (ImageEnhance, PIL image in, PIL image out) of as many 224 x 224 images
                       in `procs` single-threaded worker processes on this machine's cores, same run
  pipeline_ms_median   size_images of the whole node (two wv_image_size launches + the wv_colour_jitter call), same rounds
  ms_median / ms_min / ms_max, copy_ms_median, equal (the device batch equals the PIL pipeline's, checked before anything is
  timed)
"""
import argparse
import ctypes
import json
import multiprocessing as mp
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import _lib  # noqa: E402
from wvhash.transforms import ColorJitter, build_transform, sizing, size_images  # noqa: E402

JITTER = {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0}
NODE = {"Resize": {"size": 256}, "RandomResizedCrop": {"size": 224}, "ColorJitter": JITTER, "RandomHorizontalFlip": {"p": 0.5},
        "SWTTransform": {"level": 1, "wavelet": "haar"}}
W, H, OUT = 500, 375, 224
ALGO_BYTES = 3 * OUT * OUT * 3


def _images(n, seed, w=W, h=H):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 64, w + 64, 3), dtype=np.uint8)         # n different windows of one noise field
    return [np.ascontiguousarray(base[i % 64:i % 64 + h, (7 * i) % 64:(7 * i) % 64 + w]) for i in range(n)]


def _pillow_worker(args):
    n, seed, repeats = args
    torch.set_num_threads(1)                                                  # one core per process, none fought over
    torch.manual_seed(seed)
    imgs = [Image.fromarray(a) for a in _images(n, seed, OUT, OUT)]
    jitter = ColorJitter(**JITTER)                                            # Pillow's work alone: the three enhancements
    t0 = time.perf_counter()
    for _ in range(repeats):
        for im in imgs:
            jitter(im)
    return n * repeats, time.perf_counter() - t0


def pillow_rate(procs, per_proc=64, repeats=4):
    """images / s of `procs` processes enhancing at once: total images over the longest worker's time."""
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_pillow_worker, [(4, 0, 1)] * procs)                          # start-up and imports outside the clock
        done = pool.map(_pillow_worker, [(per_proc, p, repeats) for p in range(procs)])
    return sum(n for n, _ in done) / max(t for _, t in done)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour: needs the GPU (a rate measured elsewhere says nothing about it)")
    lib = _lib.require_gpu()
    B = args.batch
    arrays = _images(B, 1)
    tf_dev, tf_host = build_transform(NODE, defer=True, sizing="device"), build_transform(NODE, defer=True)
    check = min(B, 64)
    torch.manual_seed(3)
    ref = torch.stack([tf_host(Image.fromarray(a)) for a in arrays[:check]]).permute(0, 2, 3, 1)
    torch.manual_seed(3)                                                      # the same draws, image by image
    rb = sizing.raw_collate([tf_dev(Image.fromarray(a)) for a in arrays]).cuda()
    out = size_images(rb)
    equal = bool(torch.equal(out[:check].cpu(), ref))
    first, count, max_h, max_w = rb.colour_launches[-1]
    assert count == B and (max_h, max_w) == (OUT, OUT)                        # every image carries a chain on its last stage
    ops = ctypes.c_void_p(rb.colour.data_ptr() + first * sizing.COLOUR_WORDS * 4)
    ws_bytes = lib.wv_colour_jitter_workspace_bytes(count)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def jitter():                                                             # the last stage's images: the start of `out`
        _lib.check(lib.wv_colour_jitter(_lib.ptr(out), ops, count, max_h, max_w, _lib.ptr(ws), ctypes.c_size_t(ws_bytes),
                                        _lib.stream_ptr()), "wv_colour_jitter")

    nbytes = B * ALGO_BYTES
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for _ in range(20):                                                       # clock warm-up
        jitter()
        b.copy_(a)
        size_images(rb)
    ms, cp, pipe = [], [], []
    for _ in range(args.rounds):                                              # alternating
        ms.append(timed(jitter, args.calls))
        cp.append(timed(lambda: b.copy_(a), args.calls))
        pipe.append(timed(lambda: size_images(rb), args.calls))
    med, cmed = statistics.median(ms), statistics.median(cp)
    row = {"what": "wv_colour_jitter on 224x224 (VOC train node: brightness, contrast, saturation 0.25, random order)",
           "device": torch.cuda.get_device_name(0), "batch": B, "equal": equal, "ms_median": round(med, 4),
           "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "images_per_s": round(B / med * 1e3, 1),
           "algorithmic_bytes_per_image": ALGO_BYTES, "bytes_per_s": round(nbytes / med * 1e3, 1),
           "copy_ms_median": round(cmed, 4), "copy_bytes_per_s": round(nbytes / cmed * 1e3, 1), "copy_fraction": round(cmed / med, 4),
           "pipeline_ms_median": round(statistics.median(pipe), 4), "pillow_procs": args.procs,
           "pillow_images_per_s": round(pillow_rate(args.procs), 1)}
    row["speedup_over_pillow"] = round(row["images_per_s"] / row["pillow_images_per_s"], 1)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
