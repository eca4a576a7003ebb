"""Host-side image sizing ops that sit in front of the wavelet transform in the reference's YAML pipelines
(config/transform/basic_swt.yaml: Resize -> CenterCrop -> SWTTransform), and the plugin lookup that builds the
pipeline (Getter.get_transform, /root/reference/main/getter.py:25-35).

The reference takes Resize / CenterCrop / Compose from torchvision; torchvision is an optional dependency here
(absent -> these PIL equivalents are used: same output size rule, PIL bilinear filter like torchvision applies to
PIL images).  They decode and size images on the host; the arithmetic of the path (SWT) stays on the GPU.

With ``build_transform(cfg, defer=True, sizing="device")`` the same classes receive a ``sizing.LazyImage`` and only record
the geometry; the pixels are sized on the GPU by ``functional.size_images`` (bit-identical to Pillow, see sizing.py).
``ColorJitter`` (config/transform/voc_swt.yaml, cub_swt.yaml) records its drawn operations the same way.

``ToTensor``, ``Normalize`` and ``RandomCrop`` (config/transform/basic.yaml, cub.yaml, cub_dwt.yaml, ...) are here too;
``build_transform(cfg, defer=True)`` folds a trailing ``ToTensor [-> Normalize] [-> CustomTransform]`` into one batched plugin
step (lifting.TensorTailTransform).
"""
import math
import numbers

import torch
from PIL import Image

from .sizing import LazyImage, pil_colour


class Resize(object):
    """int size: the SHORTER side becomes `size`, aspect kept (long side = int(size * long / short));
    (h, w): exact size.  torchvision.transforms.Resize semantics for PIL input, bilinear."""

    def __init__(self, size, interpolation=Image.BILINEAR, **kwargs):
        self.size = size
        self.interpolation = interpolation

    def __call__(self, img):
        if isinstance(self.size, int) or (hasattr(self.size, "__len__") and len(self.size) == 1):
            s = self.size if isinstance(self.size, int) else self.size[0]
            w, h = img.size
            short, long = (w, h) if w <= h else (h, w)
            if short == s:
                return img
            new_short, new_long = s, int(s * long / short)
            nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
            return img.resize((nw, nh), self.interpolation)
        h, w = self.size
        return img.resize((int(w), int(h)), self.interpolation)

    def __repr__(self):
        return f"Resize(size={self.size})"


class CenterCrop(object):
    """Crop (or zero-pad, when the image is smaller) to `size` around the centre, torchvision rounding."""

    def __init__(self, size, **kwargs):
        self.size = (size, size) if isinstance(size, int) else tuple(size)

    def __call__(self, img):
        th, tw = self.size
        w, h = img.size
        if isinstance(img, LazyImage):
            # the zero-padded canvas and the crop from it as ONE window of the image: canvas origin = -(pad before)
            cw, ch = max(w, tw), max(h, th)
            left, top = int(round((cw - tw) / 2.0)) - (cw - w) // 2, int(round((ch - th) / 2.0)) - (ch - h) // 2
            return img.crop((left, top, left + tw, top + th))
        if w < tw or h < th:  # torchvision pads with zeros first
            canvas = Image.new(img.mode, (max(w, tw), max(h, th)))
            canvas.paste(img, ((max(w, tw) - w) // 2, (max(h, th) - h) // 2))
            img, (w, h) = canvas, canvas.size
        top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
        return img.crop((left, top, left + tw, top + th))

    def __repr__(self):
        return f"CenterCrop(size={self.size})"


class RandomResizedCrop(object):
    """torchvision.transforms.RandomResizedCrop for PIL input: a random rectangle of `scale` x the area and an aspect ratio
    log-uniform in `ratio`, resized to `size`.  The parameter rule is torchvision's get_params: ten attempts of
    ``torch.empty(1).uniform_`` area and log-ratio draws, sides ``int(round(sqrt(...)))``, origins from ``torch.randint``
    (row first), then the ratio-clamped centre crop.  All draws come from the torch global RNG in that order.
    torchvision is not installed where this was written: draw-for-draw parity with it is the intent and is NOT pinned
    by a test."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation=Image.BILINEAR, **kwargs):
        self.size = (size, size) if isinstance(size, int) else ((size[0], size[0]) if len(size) == 1 else tuple(size))
        self.scale, self.ratio, self.interpolation = tuple(scale), tuple(ratio), interpolation

    @staticmethod
    def get_params(width, height, scale, ratio):
        """-> (top, left, h, w)"""
        area = height * width
        log_ratio = torch.log(torch.tensor(ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = torch.randint(0, height - h + 1, size=(1,)).item()
                j = torch.randint(0, width - w + 1, size=(1,)).item()
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def __call__(self, img):
        width, height = img.size
        i, j, h, w = self.get_params(width, height, self.scale, self.ratio)
        th, tw = self.size
        return img.crop((j, i, j + w, i + h)).resize((int(tw), int(th)), self.interpolation)

    def __repr__(self):
        return f"RandomResizedCrop(size={self.size}, scale={self.scale}, ratio={self.ratio})"


class RandomCrop(object):
    """torchvision.transforms.RandomCrop for PIL input without padding: a random ``size`` window of the image.  The parameter
    rule is torchvision's get_params: no draw when the image already has the size, otherwise ``torch.randint(0, h - th + 1)``
    for the row first, then ``torch.randint(0, w - tw + 1)`` for the column, both from the torch global RNG; an image smaller
    than the crop raises ValueError.  ``padding`` / ``pad_if_needed`` other than their defaults are refused (ValueError): no
    config of the reference sets them.  Draw-for-draw parity with torchvision is the intent; parity unpinned: no test compares against
    torchvision.  On a ``sizing.LazyImage`` the crop is recorded."""

    def __init__(self, size, padding=None, pad_if_needed=False, fill=0, padding_mode="constant", **kwargs):
        if padding is not None or pad_if_needed:
            raise ValueError("RandomCrop: padding / pad_if_needed are not implemented without torchvision")
        if isinstance(size, numbers.Number):
            self.size = (int(size), int(size))
        elif len(size) == 1:
            self.size = (int(size[0]), int(size[0]))
        elif len(size) == 2:
            self.size = (int(size[0]), int(size[1]))
        else:
            raise ValueError("Please provide only two dimensions (h, w) for size.")

    @staticmethod
    def get_params(width, height, output_size):
        """-> (top, left, h, w)"""
        th, tw = output_size
        if height < th or width < tw:
            raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(height, width)}")
        if width == tw and height == th:
            return 0, 0, height, width
        i = torch.randint(0, height - th + 1, size=(1,)).item()
        j = torch.randint(0, width - tw + 1, size=(1,)).item()
        return i, j, th, tw

    def __call__(self, img):
        width, height = img.size
        i, j, h, w = self.get_params(width, height, self.size)
        return img.crop((j, i, j + w, i + h))

    def __repr__(self):
        return f"RandomCrop(size={self.size})"


class ToTensor(object):
    """torchvision.transforms.ToTensor for 8-bit images: PIL image (or uint8 ndarray [H, W] / [H, W, C]) ->
    ``float32 [C, H, W]``, the bytes divided by 255 (``.to(float32).div(255)``)."""

    def __call__(self, pic):
        import numpy as np
        if isinstance(pic, LazyImage):
            raise TypeError("ToTensor cannot run on a recorded image: build the pipeline with defer=True, which folds the tensor tail")
        if isinstance(pic, Image.Image) and pic.mode not in ("L", "P", "RGB", "RGBA", "CMYK", "YCbCr", "HSV", "LA"):
            raise TypeError(f"ToTensor: only 8-bit image modes are implemented without torchvision, got mode {pic.mode}")
        arr = np.array(pic)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3):
            raise TypeError(f"ToTensor: expected an 8-bit image, got an array of shape {arr.shape} and dtype {arr.dtype}")
        if arr.ndim == 2:
            arr = arr[:, :, None]
        return torch.from_numpy(arr).permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)

    def __repr__(self):
        return "ToTensor()"


class Normalize(object):
    """torchvision.transforms.Normalize: ``(tensor - mean[c]) / std[c]`` per channel as ``sub_`` then ``div_`` in the tensor's
    dtype (on a clone unless ``inplace``); a non-float tensor is a TypeError, a std of zero torchvision's ValueError."""

    def __init__(self, mean, std, inplace=False, **kwargs):
        self.mean, self.std, self.inplace = mean, std, inplace

    def __call__(self, tensor):
        if not isinstance(tensor, torch.Tensor):
            raise TypeError(f"img should be Tensor Image. Got {type(tensor)}")
        if not tensor.is_floating_point():
            raise TypeError(f"Input tensor should be a float tensor. Got {tensor.dtype}.")
        if tensor.ndim < 3:
            raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got tensor.size() = {tensor.size()}")
        if not self.inplace:
            tensor = tensor.clone()
        mean = torch.as_tensor(self.mean, dtype=tensor.dtype, device=tensor.device)
        std = torch.as_tensor(self.std, dtype=tensor.dtype, device=tensor.device)
        if (std == 0).any():
            raise ValueError(f"std evaluated to zero after conversion to {tensor.dtype}, leading to division by zero.")
        if mean.ndim == 1:
            mean = mean.view(-1, 1, 1)
        if std.ndim == 1:
            std = std.view(-1, 1, 1)
        return tensor.sub_(mean).div_(std)

    def __repr__(self):
        return f"Normalize(mean={self.mean}, std={self.std})"


class RandomHorizontalFlip(object):
    """Mirror left-right when ``torch.rand(1) < p`` (torchvision's rule and draw; parity unpinned like RandomResizedCrop)."""

    def __init__(self, p=0.5, **kwargs):
        self.p = p

    def __call__(self, img):
        if torch.rand(1) < self.p:
            return img.transpose(Image.FLIP_LEFT_RIGHT)
        return img

    def __repr__(self):
        return f"RandomHorizontalFlip(p={self.p})"


class ColorJitter(object):
    """torchvision.transforms.ColorJitter for PIL input: brightness, contrast, saturation (Pillow's ImageEnhance) and hue in
    a random order with random factors.
    A number v means the range [max(0, 1 - v), 1 + v] (hue: [-v, v], v <= 0.5), a pair is the range itself; a range that is
    the neutral value at both ends switches the operation off (None).  A negative number, a range outside [0, inf) (hue:
    [-0.5, 0.5]) or with its ends swapped raise ValueError, anything that is neither a number nor a pair TypeError.
    The draws are torchvision's get_params: ``torch.randperm(4)`` first, then one ``torch.empty(1).uniform_(lo, hi)`` for
    each operation that is on, in the order brightness, contrast, saturation, hue -- all from the torch global RNG.
    torchvision is not installed where this was written: draw-for-draw parity with it is the intent and is NOT pinned by
    a test.
    A ``sizing.LazyImage`` records the operations; the GPU applies them after sizing (hue is outside the kernel: such an
    image is finished with PIL in the worker)."""

    KINDS = ("brightness", "contrast", "saturation", "hue")

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, **kwargs):
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        self.hue = self._check_input(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _check_input(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError(f"If {name} is a single number, it must be non negative.")
            value = [center - float(value), center + float(value)]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            value = [float(value[0]), float(value[1])]
        else:
            raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f"{name} values should be between {bound} and in ascending order, got {value}.")
        if value[0] == value[1] == center:
            return None
        return tuple(value)

    @staticmethod
    def get_params(brightness, contrast, saturation, hue):
        """-> (order: the permutation of 0..3 as a list, then the four factors, None for an operation that is off)"""
        fn_idx = torch.randperm(4)
        drawn = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in (brightness, contrast, saturation, hue)]
        return (fn_idx.tolist(), *drawn)

    def __call__(self, img):
        order, *factors = self.get_params(self.brightness, self.contrast, self.saturation, self.hue)
        for fn_id in order:
            if factors[fn_id] is None:
                continue
            if isinstance(img, LazyImage):
                img = img.colour(self.KINDS[fn_id], factors[fn_id])
            else:
                img = pil_colour(img, self.KINDS[fn_id], factors[fn_id])
        return img

    def __repr__(self):
        return (f"ColorJitter(brightness={self.brightness}, contrast={self.contrast}, saturation={self.saturation}, "
                f"hue={self.hue})")


class Compose(object):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img

    def __repr__(self):
        return "Compose(\n" + "\n".join(f"    {t}" for t in self.transforms) + "\n)"


def build_transform(config, defer=False, device=None, sizing="host"):
    """``{name: kwargs}`` mapping (a YAML node) -> Compose, resolved like Getter.get_transform: wavelet plugins of
    this package first, then torchvision.transforms when importable, else the PIL equivalents above.
    defer / device are forwarded to the wavelet plugins (see custom_transforms.py).
    sizing="host" (default): the geometry steps resample, and ColorJitter enhances, with PIL in the worker.  sizing="device" (needs defer=True and a
    wavelet plugin at the end): they only record -- always this module's classes, which know how to --, the plugin
    returns a ``sizing.RawItem`` per image, ``sizing.raw_collate`` packs a batch and the GPU sizes it
    (``functional.size_images``): same pixels bit for bit.
    The tensor tail of the legacy configs, ``ToTensor [-> Normalize] [-> CustomTransform]`` at the END of a node, resolves
    without torchvision too (``ToTensor`` / ``Normalize`` above, ``CustomTransform`` / ``ResizeSubBands`` of lifting.py).
    With defer=True such a tail collapses into ONE plugin step, ``lifting.TensorTailTransform``: the workers hand on the
    sized uint8 pixels and ``apply_batch`` runs the whole tail on the collated batch (``functional.lift_images``; a plain
    ``ToTensor [-> Normalize]`` tail is the same call with no lifting level).  A ``ToTensor`` / ``Normalize`` /
    ``CustomTransform`` that is NOT part of such a tail (tensor steps in front of geometry) cannot be deferred: ValueError
    naming the step; with defer=False those nodes run per image."""
    from . import custom_transforms as ct
    from . import lifting
    if sizing not in ("host", "device"):
        raise ValueError(f"build_transform: sizing must be 'host' or 'device', got {sizing!r}")
    if sizing == "device" and not defer:
        raise ValueError("build_transform: sizing='device' sizes batches on the GPU after collate and needs defer=True")
    try:
        import torchvision.transforms as tvt
    except ImportError:
        tvt = None
    if sizing == "device":
        tvt = None
    local = {"Resize": Resize, "CenterCrop": CenterCrop, "RandomResizedCrop": RandomResizedCrop,
             "RandomHorizontalFlip": RandomHorizontalFlip, "ColorJitter": ColorJitter, "RandomCrop": RandomCrop,
             "ToTensor": ToTensor, "Normalize": Normalize}
    items = [(name, dict(kwargs or {})) for name, kwargs in dict(config).items()]
    extra = {"sizing": sizing} if sizing != "host" else {}
    tail = None
    if defer:
        # the tensor tail: ToTensor [-> Normalize] [-> CustomTransform] and nothing behind it
        names = [name for name, _ in items]
        for cut in (3, 2, 1):
            if tuple(names[-cut:]) in (("ToTensor", "Normalize", "CustomTransform"), ("ToTensor", "Normalize"), ("ToTensor", "CustomTransform"),
                                       ("ToTensor",)):
                folded = dict(items[-cut:])
                norm = folded.get("Normalize") or {}
                if norm.get("mean") is None and "Normalize" in folded:
                    raise TypeError("Normalize needs mean and std")
                tail = lifting.TensorTailTransform(mean=norm.get("mean"), std=norm.get("std"), custom=folded.get("CustomTransform"),
                                                   defer=True, device=device, **extra)
                items = items[:-cut]
                break
        for pos, (name, _) in enumerate(items):
            if name in ("ToTensor", "Normalize", "CustomTransform", "ResizeSubBands"):
                raise ValueError(f"build_transform: defer=True folds only a tensor tail ToTensor [-> Normalize] [-> CustomTransform] at the "
                                 f"end of the node; step {pos} '{name}' of {names} is a tensor step in front of other steps and cannot "
                                 "be deferred (build the node with defer=False)")
    steps = []
    for name, kwargs in items:
        if hasattr(ct, name) and name.endswith("Transform"):
            steps.append(getattr(ct, name)(defer=defer, device=device, **extra, **kwargs))
        elif name in ("CustomTransform", "ResizeSubBands"):
            if name == "CustomTransform" and device is not None:
                kwargs.setdefault("device", device)
            steps.append(getattr(lifting, name)(**kwargs))
        elif tvt is not None and hasattr(tvt, name):
            steps.append(getattr(tvt, name)(**kwargs))
        elif name in local:
            steps.append(local[name](**kwargs))
        else:
            raise AttributeError(f"transform '{name}' is neither a wvhash plugin nor available without torchvision")
    if tail is not None:
        steps.append(tail)
    if sizing == "device":
        if not steps or not isinstance(steps[-1], ct.BaseWaveletTransform):
            raise ValueError("build_transform: sizing='device' needs a wavelet plugin as the last step of the pipeline")
        steps.insert(0, LazyImage)
    return Compose(steps)
