"""Host-side image sizing ops that sit in front of the wavelet transform in the reference's YAML pipelines
(config/transform/basic_swt.yaml: Resize -> CenterCrop -> SWTTransform), and the plugin lookup that builds the
pipeline (Getter.get_transform, /root/reference/main/getter.py:25-35).

The reference takes Resize / CenterCrop / Compose from torchvision; torchvision is an optional dependency here
(absent -> these PIL equivalents are used: same output size rule, PIL bilinear filter like torchvision applies to
PIL images).  They decode and size images on the host; the arithmetic of the path (SWT) stays on the GPU.

With ``build_transform(cfg, defer=True, sizing="device")`` the same classes receive a ``sizing.LazyImage`` and only record
the geometry; the pixels are sized on the GPU by ``functional.size_images`` (bit-identical to Pillow, see sizing.py).
``ColorJitter`` (config/transform/voc_swt.yaml, cub_swt.yaml) records its drawn operations the same way.
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
    (``functional.size_images``): same pixels bit for bit."""
    from . import custom_transforms as ct
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
             "RandomHorizontalFlip": RandomHorizontalFlip, "ColorJitter": ColorJitter}
    steps = []
    for name, kwargs in dict(config).items():
        kwargs = dict(kwargs or {})
        if hasattr(ct, name) and name.endswith("Transform"):
            extra = {"sizing": sizing} if sizing != "host" else {}
            steps.append(getattr(ct, name)(defer=defer, device=device, **extra, **kwargs))
        elif tvt is not None and hasattr(tvt, name):
            steps.append(getattr(tvt, name)(**kwargs))
        elif name in local:
            steps.append(local[name](**kwargs))
        else:
            raise AttributeError(f"transform '{name}' is neither a wvhash plugin nor available without torchvision")
    if sizing == "device":
        if not steps or not isinstance(steps[-1], ct.BaseWaveletTransform):
            raise ValueError("build_transform: sizing='device' needs a wavelet plugin as the last step of the pipeline")
        steps.insert(0, LazyImage)
    return Compose(steps)
