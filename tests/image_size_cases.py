"""Shared by tests/test_host_image_size.py, tests/test_gpu_image_size.py and tests/golden/make_golden_image_size.py: the
size pairs of the sizing tests, seeded images, a packer that lays a ragged batch of (image, stage) pairs out for the C ABI
(independent of wvhash.transforms.sizing's recorder), and the Pillow oracle of one stage."""
import ctypes

import numpy as np
from PIL import Image, ImageOps

BILINEAR, BICUBIC = 2, 3
FILTERS = {BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}

# (w, h, out_w, out_h)
FIXED_PAIRS = [(37, 29, 16, 16), (29, 37, 48, 20), (500, 375, 341, 256), (375, 500, 256, 341), (64, 64, 224, 224),
               (640, 31, 40, 31), (33, 47, 33, 20), (225, 30, 232, 32), (17, 300, 9, 19), (2, 2, 7, 5), (1, 9, 4, 3),
               (100, 80, 6, 5)]


def random_pairs(n=150, seed=2024):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 130)), int(rng.integers(1, 130)), int(rng.integers(1, 70)), int(rng.integers(1, 70)))
            for _ in range(n)]


def image(w, h, kind, seed):
    """kind 'noise': uniform bytes; 'binary': every byte 0 or 255 (the overshoot of the bicubic lobes clips)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def stage(arr, out_wh=None, filt=BILINEAR, crop=None, window=None, flip=0):
    """One stage on image `arr` [h, w, 3]: crop (x, y, w, h) -> resize to out_wh -> window (x, y, w, h) -> flip."""
    h, w = arr.shape[:2]
    crop = crop or (0, 0, w, h)
    res = out_wh or (crop[2], crop[3])
    window = window or (0, 0, res[0], res[1])
    return {"crop": crop, "res": res, "win": window, "filter": filt, "flip": flip}


def pillow_stage(arr, st):
    """What Pillow makes of the stage: img.crop(box).resize(size, filter).crop(window) (Image.crop zero-pads outside the
    image), mirrored."""
    img = Image.fromarray(arr)
    x, y, w, h = st["crop"]
    if (x, y, w, h) != (0, 0, arr.shape[1], arr.shape[0]):
        img = img.crop((x, y, x + w, y + h))
    if st["res"] != img.size:
        img = img.resize(st["res"], FILTERS[st["filter"]])
    x, y, w, h = st["win"]
    if (x, y, w, h) != (0, 0) + img.size:
        img = img.crop((x, y, x + w, y + h))
    if st["flip"]:
        img = ImageOps.mirror(img)
    return np.array(img)


def pack(cases, stage_dtype, src_gap=0, dst_gap=0):
    """cases: [(arr, stage dict)] -> (src bytes uint8 [n], records, dst_bytes, [(dst offset, out_h, out_w)]).  Images and
    outputs lie back to back (plus `gap` bytes): ragged, mostly unaligned offsets."""
    rec = np.zeros(len(cases), dtype=stage_dtype)
    src_parts, src_off, dst_off, outs = [], 0, 0, []
    for r, (arr, st) in zip(rec, cases):
        h, w = arr.shape[:2]
        r["src_offset"], r["dst_offset"] = src_off, dst_off
        r["src_h"], r["src_w"], r["src_row_bytes"] = h, w, 3 * w
        r["crop_x"], r["crop_y"], r["crop_w"], r["crop_h"] = st["crop"]
        r["res_w"], r["res_h"] = st["res"]
        r["win_x"], r["win_y"], r["out_w"], r["out_h"] = st["win"]
        r["dst_row_bytes"], r["filter"], r["flip"] = 3 * st["win"][2], st["filter"], st["flip"]
        src_parts.append(np.ascontiguousarray(arr).reshape(-1))
        if src_gap:
            src_parts.append(np.zeros(src_gap, np.uint8))
        src_off += arr.size + src_gap
        outs.append((dst_off, st["win"][3], st["win"][2]))
        dst_off += 3 * st["win"][2] * st["win"][3] + dst_gap
    return np.concatenate(src_parts), rec, dst_off, outs


def unpack(dst, outs):
    return [dst[off:off + 3 * h * w].reshape(h, w, 3) for off, h, w in outs]


def max_ksize(rec):
    import math

    def k(i, o, f):
        return 1 if i == o else min(int(math.ceil((1.0 if f == BILINEAR else 2.0) * max(i / o, 1.0))) * 2 + 1, i)
    return max(max(k(int(r["crop_w"]), int(r["res_w"]), int(r["filter"])), k(int(r["crop_h"]), int(r["res_h"]), int(r["filter"])))
               for r in rec)


def run_cpu(lib, cases, stage_dtype):
    src, rec, dst_bytes, outs = pack(cases, stage_dtype)
    dst = np.full(dst_bytes, 0xAB, np.uint8)
    rc = lib.wv_image_size_cpu(ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data),
                               ctypes.c_void_p(rec.ctypes.data), len(rec))
    assert rc == 0, lib.wv_last_error()
    return unpack(dst, outs)


def ragged_cases():
    """The one ragged batch of the GPU test: the twelve size pairs as twelve images under both filters, plus crop-origin,
    padded-window and flip variants, one image spanning several row tiles and one on the large-scale tiling path."""
    cases = []
    for i, (w, h, ow, oh) in enumerate(FIXED_PAIRS):
        arr = image(w, h, "noise" if i % 2 == 0 else "binary", 100 + i)
        for f in (BILINEAR, BICUBIC):
            cases.append((arr, stage(arr, (ow, oh), f)))
    a = image(61, 45, "noise", 1)
    cases.append((a, stage(a, (20, 17), BILINEAR, crop=(7, 5, 40, 33))))                         # crop with an origin
    cases.append((a, stage(a, (25, 31), BICUBIC, crop=(21, 12, 40, 33))))                        # ... touching the last row / column
    cases.append((a, stage(a, (30, 22), BILINEAR, window=(-5, -3, 44, 30))))                     # window over every edge
    cases.append((a, stage(a, (30, 22), BICUBIC, window=(4, 2, 20, 40), flip=1)))                # over the bottom, mirrored
    cases.append((a, stage(a, (90, 70), BICUBIC, flip=1)))                                       # up-scale, mirrored
    cases.append((a, stage(a, None, BILINEAR, window=(-2, 40, 9, 3), flip=1)))                   # no resample at all
    cases.append((a, stage(a, None, BILINEAR, window=(70, 0, 5, 5))))                            # window beside the image: zeros
    b = image(500, 375, "noise", 2)
    cases.append((b, stage(b, (341, 256), BILINEAR, window=(58, 16, 224, 224))))                 # Resize(256) + CenterCrop(224)
    cases.append((b, stage(b, (224, 224), BILINEAR, crop=(130, 40, 301, 290), flip=1)))          # RandomResizedCrop + flip
    c = image(1920, 64, "noise", 3)
    cases.append((c, stage(c, (30, 8), BILINEAR)))                                               # 64x / 8x down: small tiles
    cases.append((c, stage(c, (30, 1), BICUBIC)))                                                # 64 rows -> 1: 257 taps
    return cases
