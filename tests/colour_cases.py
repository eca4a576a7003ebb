"""Shared by tests/test_host_colour.py, tests/test_gpu_colour.py and tests/golden/make_golden_colour.py: the chains and
images of the colour jitter tests, a packer that lays a ragged batch of (image, chain) pairs out for the C ABI (independent of
wvhash.transforms.sizing's recorder), and the Pillow oracle of one chain."""
import ctypes
import itertools

import numpy as np
from PIL import Image, ImageEnhance

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
ENHANCERS = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, SATURATION: ImageEnhance.Color}
FIXED_FACTORS = (0.0, 0.75, 1.0, 1.25, 2.0)
WIDTHS = (1, 2, 3, 4, 5, 7, 64, 223)
HEIGHTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 224)

# config/transform/voc_swt.yaml and cub_swt.yaml: the train node
VOC_TRAIN = {"Resize": {"size": 256}, "RandomResizedCrop": {"size": 224},
             "ColorJitter": {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0},
             "RandomHorizontalFlip": {"p": 0.5}}
SIZES = ((500, 375), (375, 500), (200, 180))           # the sizing tests' image sizes


def voc_node(level=1, wavelet="haar"):
    return dict(VOC_TRAIN, SWTTransform={"level": level, "wavelet": wavelet})


def orders():
    """Every subset of the three operations in every order: 1 + 3 + 6 + 6 = 16 tuples of kinds."""
    return [p for n in range(4) for p in itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION), n)]


def image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pillow_chain(arr, chain):
    """ImageEnhance applied in the chain's order: [(kind, factor), ...] on uint8 [h, w, 3]."""
    img = Image.fromarray(arr)
    for kind, factor in chain:
        img = ENHANCERS[kind](img).enhance(factor)
    return np.array(img)


def ragged_cases(seed=7):
    """[(image, chain, extra pitch bytes, gap bytes before the image)]: every order on every width; the heights, the row
    padding (0..5 bytes) and the gaps (1..3 bytes: every offset residue modulo 4) cycle.  The factors cycle through
    FIXED_FACTORS and one seeded uniform draw in [0.75, 1.25], rounded to fp32 like the descriptor holds them."""
    rng = np.random.default_rng(seed)
    cases, turn = [], 0
    for i, kinds in enumerate(orders()):
        for j, w in enumerate(WIDTHS):
            h = HEIGHTS[(i + j) % len(HEIGHTS)]
            chain = []
            for kind in kinds:
                f = FIXED_FACTORS[turn % 6] if turn % 6 < 5 else rng.uniform(0.75, 1.25)
                chain.append((kind, float(np.float32(f))))
                turn += 1
            cases.append((image(w, h, 1000 + 8 * i + j), chain, (0, 1, 2, 3, 5)[(i + 2 * j) % 5], 1 + (i + j) % 3))
    return cases


def pack(cases, dtype, fill=0xAB):
    """cases: [(arr, chain, extra pitch, gap)] or [(arr, chain)] -> (buffer uint8 [n] with the images in it and `fill`
    everywhere else, records)."""
    rec = np.zeros(len(cases), dtype=dtype)
    off = 0
    for r, case in zip(rec, cases):
        arr, chain = case[0], case[1]
        extra, gap = (case[2], case[3]) if len(case) > 2 else (0, 0)
        h, w = arr.shape[:2]
        off += gap
        r["offset"], r["h"], r["w"], r["row_bytes"], r["n_ops"] = off, h, w, 3 * w + extra, len(chain)
        for k, (kind, factor) in enumerate(chain):
            r["kind"][k], r["factor"][k] = kind, factor
        off += h * (3 * w + extra)
    buf = np.full(off, fill, np.uint8)
    for r, case in zip(rec, cases):
        place(buf, r, case[0])
    return buf, rec


def rows_view(buf, r):
    h, w, pitch, off = int(r["h"]), int(r["w"]), int(r["row_bytes"]), int(r["offset"])
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(h, 3 * w), strides=(pitch, 1))


def place(buf, r, arr):
    rows_view(buf, r)[:] = arr.reshape(arr.shape[0], -1)


def unpack(buf, rec):
    return [rows_view(buf, r).reshape(int(r["h"]), int(r["w"]), 3).copy() for r in rec]


def pillow_buffer(cases, dtype):
    """The packed buffer as it must look afterwards: every image replaced by Pillow's result, every other byte as it was."""
    buf, rec = pack(cases, dtype)
    for r, case in zip(rec, cases):
        place(buf, r, pillow_chain(case[0], case[1]))
    return buf


def run_cpu(lib, cases, dtype):
    """-> (buffer after wv_colour_jitter_cpu, records)"""
    buf, rec = pack(cases, dtype)
    rc = lib.wv_colour_jitter_cpu(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(rec.ctypes.data), len(rec))
    assert rc == 0, lib.wv_last_error()
    return buf, rec


EVAL_NODE = {"Resize": {"size": 256}, "CenterCrop": {"size": 224}, "SWTTransform": {"level": 1, "wavelet": "haar"}}


def raw_batches():
    """{name: RawBatch} of tests/golden/raw_batch_golden.npz: the VOC train node over five images (two stage indices, a
    colour table), a plain eval node (no colour table), and a recordable image beside one whose log is not (two brightness
    operations on one stage: PIL in the worker, an identity record in the batch)."""
    import torch
    from wvhash.transforms import build_transform, sizing
    out = {}
    tf = build_transform(voc_node(), defer=True, sizing="device")
    torch.manual_seed(5)
    out["voc"] = sizing.raw_collate([tf(Image.fromarray(image(*SIZES[i % 3], 60 + i))) for i in range(5)])
    tf = build_transform(EVAL_NODE, defer=True, sizing="device")
    out["eval"] = sizing.raw_collate([tf(Image.fromarray(image(w, h, 70 + w))) for w, h in ((61, 45), (45, 61), (50, 50))])
    a, b = (sizing.LazyImage(Image.fromarray(image(61, 45, 80 + i))) for i in range(2))
    a = a.resize((40, 30), Image.BICUBIC).colour("contrast", 0.75).transpose(Image.FLIP_LEFT_RIGHT)
    b = b.colour("brightness", 1.25).colour("brightness", 0.75).resize((40, 30), Image.BILINEAR)
    out["mixed"] = sizing.raw_collate([a.to_item(), b.to_item()])
    return out


def raw_batch_arrays(batches, data_limit=1 << 16):
    """The batches as the arrays the golden file holds: `data` itself up to `data_limit` bytes, its SHA-256 beyond.  The
    bytes between two images (16-byte alignment) are never written by the packer: they are zeroed here."""
    import hashlib
    from wvhash.transforms import sizing
    out = {}
    for name, rb in batches.items():
        live = np.zeros(rb.data.numel(), bool)
        for r in rb.desc.numpy().view(sizing.STAGE_DTYPE).reshape(-1)[:rb.launches[0][1]]:   # stage index 0 reads `data`
            live[int(r["src_offset"]):int(r["src_offset"]) + int(r["src_h"]) * int(r["src_row_bytes"])] = True
        data = np.where(live, rb.data.numpy(), 0).astype(np.uint8)
        if data.size <= data_limit:
            out[f"{name}_data"] = data
        else:
            out[f"{name}_data_sha256"] = np.array(hashlib.sha256(data.tobytes()).hexdigest())
        out[f"{name}_desc"] = rb.desc.numpy()
        out[f"{name}_colour"] = rb.colour.numpy() if rb.colour is not None else np.zeros((0, 12), np.int32)
        out[f"{name}_has_colour"] = np.array(rb.colour is not None)
        out[f"{name}_launches"] = np.array(rb.launches, np.int64).reshape(-1, 5)
        out[f"{name}_colour_launches"] = np.array(rb.colour_launches, np.int64).reshape(-1, 4)
        out[f"{name}_out_shape"] = np.array(rb.out_shape, np.int64)
        out[f"{name}_work_bytes"] = np.array(rb.work_bytes, np.int64)
    return out


_ALL_COLOURS = None


def all_colours():
    """One 4096 x 4096 image that holds each of the 2^24 colours once (built once, never written to)."""
    global _ALL_COLOURS
    if _ALL_COLOURS is None:
        i = np.arange(1 << 24, dtype=np.uint32)
        a = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
        a.setflags(write=False)
        _ALL_COLOURS = a
    return _ALL_COLOURS


def seeded_factor(seed):
    return float(np.float32(np.random.default_rng(seed).uniform(0.75, 1.25)))


def grey_row(values):
    """1 x n image of grey pixels: L of (v, v, v) is v, so the mean of L is the mean of `values`."""
    v = np.asarray(values, np.uint8)
    return np.repeat(v[None, :, None], 3, axis=2)


def mean_edge_images():
    """Images whose mean L is exactly x.5 or just either side of it."""
    out = [grey_row([10, 11]), grey_row([200, 201]),                    # exactly x.5: int(mean + 0.5) rounds up
           grey_row([10, 10, 11]), grey_row([10, 11, 11])]               # x.33 and x.67
    for ones in (499, 500, 501):                                         # 10.499, 10.5, 10.501
        out.append(grey_row([11] * ones + [10] * (1000 - ones)))
    return out


def golden_cases():
    """A handful of the cases above, each small: six ragged ones with all three operations, the mean edges, one order pair."""
    rag = ragged_cases()
    cases = [(c[0], c[1]) for c in rag if len(c[1]) == 3 and c[0].shape[1] in (5, 7, 64) and c[0].shape[0] <= 9][:6]
    cases += [(a, [(CONTRAST, 0.75)]) for a in mean_edge_images()[:4]]
    a = image(29, 17, 5)
    cases += [(a, [(BRIGHTNESS, 1.25), (CONTRAST, 0.75)]), (a, [(CONTRAST, 0.75), (BRIGHTNESS, 1.25)]),
              (a, [(SATURATION, seeded_factor(3))])]
    return cases
