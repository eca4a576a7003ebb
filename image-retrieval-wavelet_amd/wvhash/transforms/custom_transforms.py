"""Drop-in wavelet transform plugins: same class names, kwargs, output layout and repr as
/root/reference/main/transforms/custom_transforms.py:126-205.

Where ``SWTTransform(level, wavelet)(pil_img)`` computes (the result is always ``FloatTensor[3, 4, H', W']``):
* inside a DataLoader worker process (``torch.utils.data.get_worker_info()`` is set) -- the way the reference's
  unchanged YAML + ``DataLoader(num_workers > 0)`` calls it (flikr_coco.py:59-60) -- or with ``device="cpu"``:
  the library's host twin ``wv_swt2d_forward_cpu`` (single-threaded native code, no HIP call, fork-safe); a forked
  worker cannot use the parent's GPU context;
* in a process that owns the device: the HIP kernel (one image per call);
* no GPU and no ``device="cpu"``: ``WvhashUnavailable`` -- the transform never silently changes device.
The fast way to run the path is batched: construct with ``defer=True`` (``build_transform(cfg, defer=True)``); the
workers then only size the image and return the raw ``uint8 [3, H', W']`` tensor (16x fewer bytes over PCIe than
the expanded fp32 sub-bands), and the evaluation engine / the model run ``transform.apply_batch`` on the GPU after
collate.  A deferred batch carries no wavelet name: ``engine.evaluate`` reads it from ``dataset.transform`` and binds
the transform to the model (``model.bind_transform``); a model that receives a raw 4-D batch without a bound
transform raises instead of guessing.
With ``sizing="device"`` as well (``build_transform(cfg, defer=True, sizing="device")``) the workers do not even size the
image: the plugin returns a ``sizing.RawItem`` (decoded pixels + recorded geometry, fix_size included) and ``apply_batch``
takes the collated ``sizing.RawBatch``: sized on the GPU (``functional.size_images``), then transformed.
"""
import numpy as np
import torch
from PIL import Image
from torch.utils.data import get_worker_info

from . import functional as F
from .sizing import LazyImage


def _use_host(device, tensor=None):
    """True when a per-image call must not touch the GPU: explicit device='cpu', or a DataLoader worker process (which cannot
    use the parent's GPU context).  A tensor that already lives on the GPU stays there."""
    if tensor is not None and tensor.is_cuda:
        return False
    if device is not None and torch.device(device).type == "cpu":
        return True
    return get_worker_info() is not None


class BaseWaveletTransform(object):
    """Shared wavelet pipeline: resize to fit the level, transform each RGB channel, stack."""

    def __init__(self, level=1, wavelet='haar', defer=False, device=None, sizing="host"):
        if sizing not in ("host", "device"):
            raise ValueError(f"sizing must be 'host' or 'device', got {sizing!r}")
        if sizing == "device" and not defer:
            raise ValueError("sizing='device' needs defer=True: the batch is sized on the GPU after collate")
        self.level = level
        self.wavelet = wavelet
        self.defer = defer
        self.device = device
        self.sizing = sizing

    def fix_size(self, image):
        w, h = image.size
        factor = 2 ** self.level
        new_w = int(np.ceil(w / factor) * factor)
        new_h = int(np.ceil(h / factor) * factor)
        if new_w != w or new_h != h:
            image = image.resize((new_w, new_h), resample=Image.BICUBIC)
        return image

    def _to_u8_hwc(self, img):
        if isinstance(img, Image.Image):
            img = self.fix_size(img)
            arr = np.array(img)
        else:
            arr = np.asarray(img)
        if arr.ndim != 3 or arr.shape[2] < 3:
            raise ValueError(f"expected an RGB image (H, W, 3), got array of shape {arr.shape}")
        return np.ascontiguousarray(arr[:, :, :3])

    def _device(self):
        return torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def apply_batch(self, batch, channels_last=False, **kwargs):
        """Batched path.  batch: uint8/float32 [B,3,H,W] (or [B,H,W,3]); GPU tensors take the HIP kernel, host
        tensors the host twin.  A sizing.RawBatch (sizing="device") is sized first, where it lives."""
        raise NotImplementedError

    def apply_band(self, batch, band, channels_last=False, out_dtype=torch.float32):
        """One band of apply_batch as an image batch [B, 3, H', W']: what a single-band model reads
        (detail_tester.py:36,100 ``x[:, :, detail_index]``).  The generic form transforms and slices; SWTTransform
        computes the one band."""
        return self.apply_batch(batch, channels_last=channels_last)[:, :, band].to(out_dtype).contiguous()

    def __call__(self, img):
        """The worker-side entry of every plugin: under device sizing the recorded image (fix_size included) becomes a
        RawItem; otherwise the pixels (_to_u8_hwc) are handed on as uint8 [C, H, W] when deferred, transformed when not."""
        if self.sizing == "device":
            lazy = img if isinstance(img, LazyImage) else LazyImage(img)
            return self.fix_size(lazy).to_item()
        arr = self._to_u8_hwc(img)
        if self.defer:
            if arr.dtype != np.uint8:
                raise TypeError("deferred transforms expect 8-bit images")
            return torch.from_numpy(arr).permute(2, 0, 1).contiguous()
        if arr.dtype == np.uint8:
            x = torch.from_numpy(arr)
        else:  # the reference computes astype(float32) / 255 for any dtype
            x = torch.from_numpy(arr.astype(np.float32) / 255.0)
        x = x.unsqueeze(0)
        if _use_host(self.device):
            return self.apply_batch(x, channels_last=True)[0]
        from .. import _lib
        try:
            _lib.require_gpu()
        except _lib.WvhashUnavailable as e:
            raise _lib.WvhashUnavailable(f"{e}; pass device='cpu' to run the library's host twin in this process "
                                         "(DataLoader workers take it automatically)") from None
        return self.apply_batch(x.to(self._device(), non_blocking=True), channels_last=True)[0].cpu().float()

    def deferred_spec(self):
        """What a deferred batch needs to be expanded later: (kind, wavelet, level, copies)."""
        return (type(self).__name__, self.wavelet, self.level, getattr(self, "copies", 4))


def find_wavelet_transform(obj):
    """The wavelet plugin inside a transform pipeline (a plugin itself, a Compose-like object with a
    ``transforms`` list, a dataset with a ``transform`` attribute, or a wrapper such as torch.utils.data.Subset holding
    one in ``dataset``); None when there is none."""
    if isinstance(obj, BaseWaveletTransform):
        return obj
    for attr in ("transform", "transforms", "dataset"):
        inner = getattr(obj, attr, None)
        if inner is None:
            continue
        if isinstance(inner, (list, tuple)):
            for t in inner:
                found = find_wavelet_transform(t)
                if found is not None:
                    return found
        else:
            found = find_wavelet_transform(inner)
            if found is not None:
                return found
    return None


class SWTTransform(BaseWaveletTransform):
    """Stationary wavelet transform (size preserved: H, W)."""

    def apply_batch(self, batch, channels_last=False, **kwargs):
        batch, channels_last = F.sized(batch, channels_last)
        if not batch.is_cuda:
            return F.swt2d_host(batch, self.wavelet, self.level, channels_last=channels_last)
        return F.swt2d(batch, self.wavelet, self.level, channels_last=channels_last, **kwargs)

    def apply_band(self, batch, band, channels_last=False, out_dtype=torch.float32):
        batch, channels_last = F.sized(batch, channels_last)
        if not batch.is_cuda:
            return F.swt2d_band_host(batch, self.wavelet, self.level, band, channels_last=channels_last).to(out_dtype)
        return F.swt2d_band(batch, self.wavelet, self.level, band, channels_last=channels_last, out_dtype=out_dtype)

    def __repr__(self):
        return f"SWTTransform(shape='C,S,H,W', wavelet={self.wavelet}, level={self.level})"


class RawStackTransform(BaseWaveletTransform):
    """Parameter-matched control: every 'subband' is an identical copy of the raw channel."""

    def __init__(self, level=1, wavelet='haar', copies=4, defer=False, device=None, sizing="host"):
        super().__init__(level=level, wavelet=wavelet, defer=defer, device=device, sizing=sizing)
        self.copies = copies

    def apply_batch(self, batch, channels_last=False, **kwargs):
        batch, channels_last = F.sized(batch, channels_last)
        if not batch.is_cuda:
            return F.rawstack_host(batch, self.copies, channels_last=channels_last)
        return F.rawstack(batch, self.copies, channels_last=channels_last)

    def __repr__(self):
        return f"RawStackTransform(shape='C,{self.copies},H,W', copies={self.copies})"


class DWTTransform(BaseWaveletTransform):
    """Discrete multi-level wavelet transform (size divided by 2^level): the coarsest-level bands of
    ``pywt.wavedec2`` with PyWavelets' default symmetric extension (a plain, untuned kernel: this
    transform is outside the hot path)."""

    def __init__(self, level=1, wavelet='haar', defer=False, device=None, sizing="host"):
        super().__init__(level=level, wavelet=wavelet, defer=defer, device=device, sizing=sizing)

    def apply_batch(self, batch, channels_last=False, **kwargs):
        batch, channels_last = F.sized(batch, channels_last)
        if not batch.is_cuda:
            return F.dwt2d_host(batch, self.wavelet, self.level, channels_last=channels_last)
        return F.dwt2d(batch, self.wavelet, self.level, channels_last=channels_last)

    def __repr__(self):
        factor = 2 ** self.level
        return f"DWTTransform(shape='C,S,H/{factor},W/{factor}', wavelet={self.wavelet}, level={self.level})"
