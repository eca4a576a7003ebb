"""Shared by tests/test_host_lifting.py and tests/test_gpu_lifting_batched.py: the transform nodes of the legacy configs, the
expected values of the tensor tail (live torch ops for ToTensor / Normalize, oracle.lifting_np for the lifting), and the
ctypes calls of the C ABI."""
import ctypes

import numpy as np
import torch
from PIL import Image

from oracle import lifting_np

BASES = ("haar", "cdf97")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
UNEQUAL = ((0.5, 0.25, 0.125), (0.5, 2.0, 3.0))
# every residue mod 4; axes shorter than the cdf 9/7 stencil; sizes that turn odd in the cascade (100 x 75, 50 x 30)
SMALL = (1, 2, 3, 4, 5, 7, 8, 9, 13, 18, 30, 50, 75, 100)

_NORM = {"mean": list(IMAGENET[0]), "std": list(IMAGENET[1])}
_JITTER = {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0.0}
_HAAR1 = {"decompose_levels": 1, "basis": "haar", "coarse_only": True, "ll_only": False}
_CDF1 = {"decompose_levels": 1, "basis": "cdf97", "coarse_only": False}
# config/transform/cub_dwt.yaml, cub_dwt_cdf97.yaml, basic.yaml, sdd_dwt.yaml
CUB_DWT = {
    "train": {"Resize": {"size": 256}, "RandomResizedCrop": {"scale": [0.16, 1], "ratio": [0.75, 1.33], "size": 224}, "ColorJitter": _JITTER,
              "RandomHorizontalFlip": {"p": 0.5}, "ToTensor": {}, "Normalize": _NORM, "CustomTransform": _HAAR1},
    "test": {"Resize": {"size": 256}, "CenterCrop": {"size": 224}, "ToTensor": {}, "Normalize": _NORM, "CustomTransform": _HAAR1}}
CUB_DWT_CDF97 = {
    "train": {"RandomResizedCrop": {"size": 448, "scale": [0.16, 1.0], "ratio": [0.75, 1.33]}, "ColorJitter": _JITTER,
              "RandomHorizontalFlip": {"p": 0.5}, "ToTensor": {}, "Normalize": _NORM, "CustomTransform": _CDF1},
    "test": {"Resize": {"size": 512}, "CenterCrop": {"size": 448}, "ToTensor": {}, "Normalize": _NORM, "CustomTransform": _CDF1}}
BASIC = {"train": {"Resize": {"size": 256}, "RandomCrop": {"size": 224}, "RandomHorizontalFlip": {"p": 0.5}, "ToTensor": {}},
         "test": {"Resize": {"size": 256}, "CenterCrop": {"size": 224}, "ToTensor": {}}}
SDD_DWT_TRAIN = {"ToTensor": {}, "CustomTransform": {"decompose_levels": 1, "basis": "haar"}, "Resize": {"size": [256, 256]},
                 "RandomCrop": {"size": [224, 224]}, "RandomHorizontalFlip": {"p": 0.5}}
IMAGE_SIZES = ((500, 375), (375, 500), (300, 260), (256, 256), (640, 480), (281, 333))      # (w, h)


def pil_images(n, seed=11):
    """n synthetic RGB images of different sizes: smooth gradients plus noise, so that resampling has something to do."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w, h = IMAGE_SIZES[k % len(IMAGE_SIZES)]
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 255 // (w + h))], axis=2)
        arr = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
        out.append(Image.fromarray(arr))
    return out


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def to_tensor_normalize(x_nchw_u8, mean=None, std=None):
    """Live torch ops, as ToTensor and Normalize run them: uint8 [B,C,H,W] -> float32."""
    t = torch.as_tensor(x_nchw_u8).to(dtype=torch.float32).div(255)
    if mean is not None:
        m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
        s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
        t = t.sub_(m).div_(s)
    return t


def expected(t_nchw, basis, levels, ll_only):
    """float32 [B,C,H,W] (already converted) -> what wv_lift_images must return, by the oracle."""
    t = np.asarray(t_nchw, dtype=np.float32)
    if levels == 0:
        return t
    return lifting_np.custom_transform(t, levels, basis, coarse_only=True, ll_only=bool(ll_only))


def out_shape(lib, B, C, H, W, basis, levels, ll_only):
    b = BASES.index(basis)
    h, w = (lib.wv_lift_out_size(H, b, levels), lib.wv_lift_out_size(W, b, levels)) if levels else (H, W)
    return (B, C, h, w) if levels == 0 or ll_only else (B, C, 4, h, w)


def floats(values):
    return None if values is None else (ctypes.c_float * len(values))(*values)


def nhwc(x_nchw):
    return np.ascontiguousarray(np.asarray(x_nchw).transpose(0, 2, 3, 1))


def run_cpu(lib, x, layout, B, C, H, W, mean, std, basis, levels, ll_only, to_tensor=None):
    """wv_lift_images_cpu on a numpy array laid out as `layout` says -> (rc, out)."""
    x = np.ascontiguousarray(x)
    dt = 0 if x.dtype == np.uint8 else 1
    out = np.full(out_shape(lib, B, C, H, W, basis, levels, ll_only), np.nan, np.float32)
    rc = lib.wv_lift_images_cpu(ctypes.c_void_p(x.ctypes.data), dt, layout, B, C, H, W, int(dt == 0) if to_tensor is None else to_tensor,
                                floats(mean), floats(std), BASES.index(basis), levels, int(ll_only), ctypes.c_void_p(out.ctypes.data))
    return rc, out
