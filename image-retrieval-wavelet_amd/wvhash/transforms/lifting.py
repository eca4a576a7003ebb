"""Legacy lifting-scheme transforms with the reference's names and call conventions
(/root/reference/main/transforms/custom_transforms.py:14-117): ``HaarLifting``, ``Cdf97Lifting``, ``ResizeSubBands``,
``CustomTransform(decompose_levels, basis, coarse_only, ll_only)``.  The lifting arithmetic runs in libwvhash, bit-identical
to the reference's float32 torch ops: the lifting modules pad on the host and run one ``wv_lifting2d_forward`` per level,
``CustomTransform`` is one ``wv_lift_images`` call over the planes.  Inputs are float tensors ``[C, H, W]`` or ``[N, C, H, W]``
(what ToTensor / Normalize hand over); a CPU tensor is moved to the GPU for the call and the result comes back on its
original device, so the classes also work as a per-image transform in a ``num_workers=0`` pipeline.  With ``device="cpu"``, or
inside a DataLoader worker, ``CustomTransform`` takes the library's host twin instead (``wv_lift_images_cpu``: same bits, no
GPU touched).

The batched form is ``TensorTailTransform``: the whole tensor tail ``ToTensor [-> Normalize] [-> CustomTransform]`` of a
deferred pipeline as one plugin step whose ``apply_batch`` is one ``wv_lift_images`` call on the sized uint8 batch.
"""
import ctypes
from collections.abc import Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from . import functional as Fn
from .custom_transforms import BaseWaveletTransform, _use_host


def lifting2d(x, basis):
    """One level on the GPU.  x: float32 CUDA [..., H, W] with H, W even -> (ll [..., H/2, W/2], hi [..., 3, H/2, W/2])."""
    lib = _lib.require_gpu()
    if not x.is_cuda:
        raise ValueError("lifting2d: input must live on the GPU (no CPU path in the product)")
    x = x.float().contiguous()
    *lead, H, W = x.shape
    planes = 1
    for d in lead:
        planes *= d
    ll = torch.empty((*lead, H // 2, W // 2), dtype=torch.float32, device=x.device)
    hi = torch.empty((*lead, 3, H // 2, W // 2), dtype=torch.float32, device=x.device)
    if planes == 0:
        return ll, hi
    ws_bytes = lib.wv_lifting2d_workspace_bytes(planes, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.wv_lifting2d_forward(_lib.ptr(x), planes, H, W, Fn.LIFT_BASIS[basis], _lib.ptr(ll), _lib.ptr(hi), _lib.ptr(ws),
                                      ctypes.c_size_t(ws_bytes), _lib.stream_ptr())
        _lib.check(rc, "wv_lifting2d_forward")
    return ll, hi


class _Lifting(nn.Module):
    basis = "haar"

    def __init__(self, n_levels=1, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.n_levels = n_levels

    def _pad(self, x):
        raise NotImplementedError

    def forward_one(self, x):
        return lifting2d(self._pad(x), self.basis)

    def forward(self, x):
        dev = x.device
        if not x.is_cuda:
            _lib.require_gpu()
            x = x.cuda()
        details, approx = [], []
        for _ in range(self.n_levels):
            x, high = self.forward_one(x)
            details.append(high.to(dev))
            approx.append(x.to(dev))
        return approx, details


class HaarLifting(_Lifting):
    basis = "haar"

    def _pad(self, x):
        h, w = x.shape[-2:]
        return F.pad(x, (0, w % 2, 0, h % 2))


class Cdf97Lifting(_Lifting):
    basis = "cdf97"

    def _pad(self, x):
        h, w = x.shape[-2:]
        return F.pad(x, (0, (4 - (w % 4)) % 4, 0, (4 - (h % 4)) % 4))


class ResizeSubBands(nn.Module):
    """Bilinear (antialiased) resize of a sub-band tensor: ``torchvision.transforms.functional.resize`` on tensors is
    ``torch.nn.functional.interpolate`` underneath, which is what runs here (torchvision is optional)."""

    def __init__(self, size, interpolation="bilinear", max_size=None, antialias=True):
        super().__init__()
        ok = isinstance(size, int) or (isinstance(size, Sequence) and len(size) in (1, 2)
                                       and all(isinstance(v, int) for v in size))
        if not ok:
            raise (TypeError if not isinstance(size, (int, Sequence)) else ValueError)(
                f"ResizeSubBands: size must be an int or a sequence of one or two ints, got {size!r}")
        self.size, self.max_size, self.antialias = size, max_size, antialias
        self.interpolation = getattr(interpolation, "value", interpolation)

    def forward(self, img):
        h, w = img.shape[-2:]
        size = self.size
        if isinstance(size, int) or len(size) == 1:            # shorter side -> size, aspect kept
            s = size if isinstance(size, int) else size[0]
            short, long = (w, h) if w <= h else (h, w)
            new_short, new_long = s, int(s * long / short)
            if self.max_size is not None and new_long > self.max_size:
                new_short, new_long = int(self.max_size * new_short / new_long), self.max_size
            size = (new_long, new_short) if w <= h else (new_short, new_long)
        lead = img.shape[:-2]
        x = img.reshape(-1, 1, h, w).float()
        y = F.interpolate(x, size=tuple(size), mode=self.interpolation, align_corners=False if self.interpolation != "nearest" else None,
                          antialias=self.antialias and self.interpolation in ("bilinear", "bicubic"))
        return y.reshape(*lead, *size).to(img.dtype)


WAVELET_DICT = {"haar": HaarLifting, "cdf97": Cdf97Lifting}


def _refuse_unstackable(levels, coarse_only, ll_only):
    if not coarse_only and levels > 1:      # levels have different sizes: nothing to stack (the reference raises as well)
        raise NotImplementedError(f"Full {'approx' if ll_only else 'subbands'} not implemented yet for decompose_levels > 1 ")


class CustomTransform:
    """Tensor-side lifting DWT of the legacy CNN configs (custom_transforms.py:90-117).  Output by option pair:

    ==========  ===========  ==============================================================
    ll_only     coarse_only  result (band axis = dim -3)
    ==========  ===========  ==============================================================
    False       True         coarsest level: approximation stacked on its three detail bands
    False       False        every level's bands stacked (single-level decompositions only)
    True        True         coarsest approximation alone
    True        False        every level's approximation stacked (single level only)
    ==========  ===========  ==============================================================
    """

    def __init__(self, decompose_levels=3, basis="haar", coarse_only=True, ll_only=False, device='cuda', dwt_mode='dwt'):
        self.dwt = WAVELET_DICT[basis](n_levels=decompose_levels)
        self.decompose_levels, self.basis, self.device = decompose_levels, basis, device
        self.coarse_only, self.ll_only = coarse_only, ll_only

    def __call__(self, img):
        # what is left is stackable, and then every option pair is the coarsest level's bands
        _refuse_unstackable(self.decompose_levels, self.coarse_only, self.ll_only)
        *lead, H, W = img.shape
        planes = img.float().reshape(-1, 1, H, W)
        kwargs = dict(basis=self.basis, levels=self.decompose_levels, ll_only=self.ll_only)
        if _use_host(self.device, img):
            out = Fn.lift_images_host(planes, **kwargs)
        else:
            _lib.require_gpu()
            out = Fn.lift_images(planes if planes.is_cuda else planes.cuda(), **kwargs).to(img.device)
        return out.reshape(*lead, *out.shape[2:])


class TensorTailTransform(BaseWaveletTransform):
    """The deferred form of a pipeline's tensor tail, ``ToTensor [-> Normalize] [-> CustomTransform]``, as ONE plugin step
    (``build_transform(cfg, defer=True)`` folds the tail into it).  Per image it only hands the sized pixels on --
    ``uint8 [C, H, W]`` under host sizing, a ``sizing.RawItem`` under device sizing; nothing is resized to fit a level (the
    lifting pads with zeros, there is no ``fix_size``).  ``apply_batch`` runs the whole tail on the collated batch:
    ``functional.sized`` then ``functional.lift_images`` (``lift_images_host`` for host tensors), bit-identical to the
    per-image torch ops.  ``custom`` = CustomTransform's kwargs, or None for a plain ``ToTensor [-> Normalize]`` tail
    (levels = 0: float32 ``[B, C, H, W]``)."""

    def __init__(self, mean=None, std=None, custom=None, defer=True, device=None, sizing="host"):
        custom = None if custom is None else dict(custom)
        levels = 0 if custom is None else int(custom.get("decompose_levels", 3))
        basis = "haar" if custom is None else custom.get("basis", "haar")
        if basis not in Fn.LIFT_BASIS:
            raise KeyError(basis)
        if not defer:
            raise ValueError("TensorTailTransform is the deferred form of the tail; with defer=False the steps run per image")
        super().__init__(level=levels, wavelet=basis, defer=True, device=device, sizing=sizing)
        self.ll_only = bool(custom.get("ll_only", False)) if custom else False
        _refuse_unstackable(levels, custom is None or custom.get("coarse_only", True), self.ll_only)
        if (mean is None) != (std is None):
            raise ValueError("Normalize needs mean and std")
        self.mean = None if mean is None else tuple(float(v) for v in mean)
        self.std = None if std is None else tuple(float(v) for v in std)
        if self.std is not None and any(torch.tensor(v, dtype=torch.float32) == 0 for v in self.std):
            raise ValueError("std evaluated to zero after conversion to torch.float32, leading to division by zero.")
        self.custom = custom

    def fix_size(self, image):
        return image

    def _to_u8_hwc(self, img):
        arr = np.array(img)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3):
            raise TypeError(f"deferred ToTensor expects an 8-bit image, got an array of shape {arr.shape} and dtype {arr.dtype}")
        return np.ascontiguousarray(arr if arr.ndim == 3 else arr[:, :, None])

    def apply_batch(self, batch, channels_last=False, **kwargs):
        batch, channels_last = Fn.sized(batch, channels_last)
        if batch.dim() != 4:
            raise ValueError(f"expected a 4-D batch, got shape {tuple(batch.shape)}")
        C = batch.shape[3] if channels_last else batch.shape[1]
        m, s = self.mean, self.std
        if m is not None and len(m) == 1 and C > 1:              # Normalize broadcasts one value over the channels
            m, s = m * C, s * C
        fn = Fn.lift_images if batch.is_cuda else Fn.lift_images_host
        return fn(batch, m, s, basis=self.wavelet, levels=self.level, ll_only=self.ll_only, channels_last=channels_last)

    def __repr__(self):
        steps = ["ToTensor()"]
        if self.mean is not None:
            steps.append(f"Normalize(mean={self.mean}, std={self.std})")
        if self.custom is not None:
            steps.append(f"CustomTransform(decompose_levels={self.level}, basis={self.wavelet}, "
                         f"coarse_only={self.custom.get('coarse_only', True)}, ll_only={self.ll_only})")
        return "TensorTailTransform(" + " -> ".join(steps) + ")"
