"""Batched device-side wavelet transforms (the HIP path behind the plugin classes)."""
import ctypes

import torch

from .. import _lib
from .sizing import COLOURS, STAGES, RawBatch
from .wavelets import get_filters

LIFT_BASIS = {"haar": 0, "cdf97": 1}


def _layout_and_shape(x, channels_last):
    if x.dim() != 4:
        raise ValueError(f"expected a 4-D batch, got shape {tuple(x.shape)}")
    if channels_last:
        B, H, W, C = x.shape
        return _lib.WV_LAYOUT_NHWC, B, C, H, W
    B, C, H, W = x.shape
    return _lib.WV_LAYOUT_NCHW, B, C, H, W


def _batch(x, channels_last, what, on_gpu, note):
    """The preamble of every wrapper below -> (x contiguous, layout, B, C, H, W); x must live where `what` runs."""
    if x.is_cuda != on_gpu:
        raise ValueError(f"{what}: input must live on the GPU{note}" if on_gpu else f"{what}: the host twin takes host tensors ({note})")
    x = x.contiguous()
    return (x,) + _layout_and_shape(x, channels_last)


_HOST_NOTE = "use the device function for GPU tensors"


def _swt_size(H, W, level):
    if H % (1 << level) or W % (1 << level):
        # PyWavelets' message for swt2 on a bad size
        raise ValueError(f"Length of data must be even along the transform axis / divisible by 2**level; "
                         f"got {H}x{W} at level {level}")


def _in_dtype(x):
    if x.dtype == torch.uint8:
        return _lib.WV_DT_U8
    if x.dtype == torch.float32:
        return _lib.WV_DT_F32
    raise TypeError(f"images must be uint8 (0..255) or float32 (already scaled), got {x.dtype}")


def _size_launches(raw_batch, call, work, colour_call):
    colour_launches = raw_batch.colour_launches
    for s, (first, count, max_h, max_w, max_k) in enumerate(raw_batch.launches):
        src = raw_batch.data if s == 0 else work          # later stages read what earlier ones wrote
        call(_lib.ptr(src), _lib.ptr(work), STAGES.address(raw_batch.desc, first), count, max_h, max_w, max_k)
        if s < len(colour_launches) and colour_launches[s][1]:
            first, count, max_h, max_w = colour_launches[s]  # the colour chains of what this stage wrote, in place
            colour_call(_lib.ptr(work), COLOURS.address(raw_batch.colour, first), count, max_h, max_w)
    B, H, W = raw_batch.out_shape
    return work[:B * H * W * 3].view(B, H, W, 3)


def size_images(raw_batch):
    """sizing.RawBatch on the GPU -> uint8 [B, H, W, 3]: crop, resample (Pillow's 8-bit BILINEAR / BICUBIC bit for bit),
    window / zero pad and mirror of every image, one wv_image_size launch per stage index on the current stream; the
    intermediate images of pipelines with two resamples live in the same freshly allocated buffer as the result.  The
    colour chains recorded on a stage (ColorJitter; Pillow's ImageEnhance bit for bit) follow its launch as one
    wv_colour_jitter call, in place."""
    lib = _lib.require_gpu()
    if not raw_batch.is_cuda:
        raise ValueError("size_images: the batch must live on the GPU (size_images_host is the host twin)")
    if raw_batch.desc.dtype != torch.int32 or not raw_batch.desc.is_contiguous() or not raw_batch.data.is_contiguous():
        raise ValueError("size_images: descriptor tensor must be contiguous int32, data contiguous uint8")
    colour = raw_batch.colour
    if colour is not None and (colour.dtype != torch.int32 or not colour.is_contiguous() or colour.device != raw_batch.device):
        raise ValueError("size_images: colour descriptor tensor must be contiguous int32 on the batch's device")
    work = torch.empty(raw_batch.work_bytes, dtype=torch.uint8, device=raw_batch.device)

    def call(src, dst, stages, count, max_h, max_w, max_k):
        _lib.check(lib.wv_image_size(src, dst, stages, count, max_h, max_w, max_k, _lib.stream_ptr()), "wv_image_size")

    def colour_call(img, ops, count, max_h, max_w):
        nbytes = lib.wv_colour_jitter_workspace_bytes(count)
        sums = torch.empty(nbytes, dtype=torch.uint8, device=raw_batch.device)
        _lib.check(lib.wv_colour_jitter(img, ops, count, max_h, max_w, _lib.ptr(sums), ctypes.c_size_t(nbytes), _lib.stream_ptr()),
                   "wv_colour_jitter")

    with torch.cuda.device(raw_batch.device):
        return _size_launches(raw_batch, call, work, colour_call)


def size_images_host(raw_batch):
    """Host twin of size_images (wv_image_size_cpu, wv_colour_jitter_cpu): the same bytes from a RawBatch of host tensors."""
    lib = _lib.load()
    if raw_batch.is_cuda:
        raise ValueError("size_images_host: the host twin takes host tensors (size_images is the device function)")
    work = torch.empty(raw_batch.work_bytes, dtype=torch.uint8)

    def call(src, dst, stages, count, max_h, max_w, max_k):
        _lib.check(lib.wv_image_size_cpu(src, dst, stages, count), "wv_image_size_cpu")

    def colour_call(img, ops, count, max_h, max_w):
        _lib.check(lib.wv_colour_jitter_cpu(img, ops, count), "wv_colour_jitter_cpu")

    return _size_launches(raw_batch, call, work, colour_call)


def sized(batch, channels_last):
    """(batch, channels_last) with a sizing.RawBatch replaced by its sized uint8 [B, H, W, 3] images (on the GPU when it
    lives there, by the host twin otherwise); tensors pass through."""
    if isinstance(batch, RawBatch):
        return (size_images(batch) if batch.is_cuda else size_images_host(batch)), True
    return batch, channels_last


def swt2d(x, wavelet="haar", level=1, channels_last=False, out_dtype=torch.float32, out=None, band_major=False):
    """Batch of images on the GPU -> [B, C, 4, H, W] level-`level` sub-bands (cA, cH, cV, cD).

    Same numbers as stacking ``SWTTransform(level, wavelet)(img)`` of the reference
    (custom_transforms.py:145-166) over the batch: uint8 input is divided by 255 in fp32,
    float32 input is used as is.  ``channels_last`` = the batch is [B, H, W, C] (PIL layout).
    ``out`` = preallocated result buffer (reused across steps, e.g. when the transform runs on its own stream).
    ``band_major`` = write ``[4, B, C, H, W]`` instead: every band is one contiguous NCHW batch, so the models'
    band split (multi_dino_attention.py:818 ``permute(2,0,1,3,4).contiguous()``, :745 ``x[..., i, :, :]``) is a
    view and the sub-band tensor is never copied a second time.
    """
    lib = _lib.require_gpu()
    x, layout, B, C, H, W = _batch(x, channels_last, "swt2d", True, " (swt2d_host is the host twin)")
    lo, hi = get_filters(wavelet)
    odt = _out_dtype(out_dtype)
    shape = (4, B, C, H, W) if band_major else (B, C, 4, H, W)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"swt2d: `out` must be a contiguous {list(shape)} tensor of out_dtype on the input's device")
    if B == 0:
        return out
    _swt_size(H, W, level)
    ws_bytes = lib.wv_swt2d_workspace_bytes(B, C, H, W, level, len(lo))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    flo, fhi = _lib.host_floats(lo), _lib.host_floats(hi)
    with torch.cuda.device(x.device):
        for b0 in range(0, B, 65535):
            b1 = min(B, b0 + 65535)
            if band_major:
                rc = lib.wv_swt2d_forward_ex(_lib.ptr(x[b0:b1]), _in_dtype(x), layout, _lib.ptr(out[0, b0:b1]), odt,
                                             _lib.WV_BANDS_OUTER, B * C * H * W, b1 - b0, C, H, W, level, flo, fhi,
                                             len(lo), _lib.ptr(ws), ctypes.c_size_t(ws_bytes), _lib.stream_ptr())
                if rc == _lib.WV_ENOTSUP:     # shape outside the sliding kernel -> reference layout, re-laid out once
                    inner = swt2d(x, wavelet, level, channels_last=channels_last, out_dtype=out_dtype)
                    out.copy_(inner.permute(2, 0, 1, 3, 4))
                    return out
                _lib.check(rc, "wv_swt2d_forward_ex")
            else:
                rc = lib.wv_swt2d_forward(_lib.ptr(x[b0:b1]), _in_dtype(x), layout, _lib.ptr(out[b0:b1]), odt,
                                          b1 - b0, C, H, W, level, flo, fhi, len(lo), _lib.ptr(ws),
                                          ctypes.c_size_t(ws_bytes), _lib.stream_ptr())
                _lib.check(rc, "wv_swt2d_forward")
    return out


def _out_dtype(out_dtype):
    if out_dtype == torch.float32:
        return _lib.WV_DT_F32
    if out_dtype == torch.bfloat16:
        return _lib.WV_DT_BF16
    raise TypeError("out_dtype must be float32 or bfloat16")


def swt2d_band(x, wavelet="haar", level=1, band=0, channels_last=False, out_dtype=torch.float32, out=None):
    """Batch of images on the GPU -> [B, C, H, W]: band `band` (0..3 = cA, cH, cV, cD) of the level-`level` SWT, the
    tensor a single-band model reads (detail_tester.py:36,100 ``x[:, :, detail_index]``), bit-identical to
    ``swt2d(...)[:, :, band]``.  On the sliding kernel's shapes only that band is computed and written
    (wv_swt2d_band_forward); any other shape is the four-band transform and a slice."""
    lib = _lib.require_gpu()
    x, layout, B, C, H, W = _batch(x, channels_last, "swt2d_band", True, " (swt2d_band_host is the host twin)")
    lo, hi = get_filters(wavelet)
    odt = _out_dtype(out_dtype)
    band = int(band)
    if not 0 <= band <= 3:
        raise ValueError(f"swt2d_band: band must be 0..3 (cA, cH, cV, cD), got {band}")
    shape = (B, C, H, W)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"swt2d_band: `out` must be a contiguous {list(shape)} tensor of out_dtype on the input's device")
    if B == 0:
        return out
    _swt_size(H, W, level)
    flo, fhi = _lib.host_floats(lo), _lib.host_floats(hi)
    with torch.cuda.device(x.device):
        for b0 in range(0, B, 65535):
            b1 = min(B, b0 + 65535)
            rc = lib.wv_swt2d_band_forward(_lib.ptr(x[b0:b1]), _in_dtype(x), layout, _lib.ptr(out[b0:b1]), odt, band,
                                           b1 - b0, C, H, W, level, flo, fhi, len(lo), _lib.stream_ptr())
            if rc == _lib.WV_ENOTSUP:     # shape outside the sliding kernel -> all four bands, sliced once
                inner = swt2d(x, wavelet, level, channels_last=channels_last, out_dtype=out_dtype)
                out.copy_(inner[:, :, band])
                return out
            _lib.check(rc, "wv_swt2d_band_forward")
    return out


def swt2d_place_output(x, wavelet="haar", level=1, channels_last=False, out_dtype=torch.float32, band_major=False,
                       candidates=8, launches=4, first=None):
    """A result buffer for swt2d(x, ..., out=buffer) placed where the kernel runs fastest, for callers that keep one buffer
    for many batches of x's shape (a serving loop, bench.py).  WHERE a multi-GB write target lies in HBM moves the kernel by
    about +-3 % (the first large allocation of a process up to +10 %; one allocation behaves the same at every offset inside
    it -- DESIGN.md 5), so `candidates` buffers are allocated side by side, the transform is timed on each (`launches`
    launches, HIP events on the current stream) and the fastest is returned; the others go back to the driver.
    `first`: a buffer of the right shape the caller already holds; it is candidate 0.
    -> (buffer, {"candidates", "probe_ms", "picked"})."""
    _lib.require_gpu()
    layout, B, C, H, W = _layout_and_shape(x.contiguous(), channels_last)
    shape = (4, B, C, H, W) if band_major else (B, C, 4, H, W)
    if first is not None and (tuple(first.shape) != shape or first.dtype != out_dtype or first.device != x.device):
        raise ValueError("swt2d_place_output: `first` does not have the output's shape / dtype / device")
    bufs, ms = [], []
    for c in range(max(1, int(candidates))):
        buf = first if (c == 0 and first is not None) else torch.empty(shape, dtype=out_dtype, device=x.device)
        bufs.append(buf)
        if candidates <= 1 or B == 0:
            break
        for _ in range(2):
            swt2d(x, wavelet, level, channels_last=channels_last, out_dtype=out_dtype, out=buf, band_major=band_major)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            swt2d(x, wavelet, level, channels_last=channels_last, out_dtype=out_dtype, out=buf, band_major=band_major)
        e1.record()
        torch.cuda.synchronize(x.device)
        ms.append(round(e0.elapsed_time(e1) / launches, 4))
    pick = ms.index(min(ms)) if ms else 0
    best = bufs[pick]
    del bufs, buf
    torch.cuda.empty_cache()
    return best, {"candidates": max(1, int(candidates)), "probe_ms": ms, "picked": pick}


def dwt2d(x, wavelet="haar", level=1, channels_last=False):
    """Batch of images on the GPU -> [B, C, 4, H', W'] coarsest-level bands of the decimated DWT
    (``pywt.wavedec2(..., mode='symmetric')``, DWTTransform at custom_transforms.py:197-201)."""
    lib = _lib.require_gpu()
    x, layout, B, C, H, W = _batch(x, channels_last, "dwt2d", True, " (no CPU path in the product)")
    lo, hi = get_filters(wavelet)
    Hn, Wn = lib.wv_dwt_out_len(H, len(lo), level), lib.wv_dwt_out_len(W, len(lo), level)
    out = torch.empty((B, C, 4, Hn, Wn), dtype=torch.float32, device=x.device)
    if B == 0:
        return out
    ws_bytes = lib.wv_dwt2d_workspace_bytes(B, C, H, W, level, len(lo))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.wv_dwt2d_forward(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), B, C, H, W, level,
                                  _lib.host_floats(lo), _lib.host_floats(hi), len(lo), _lib.ptr(ws),
                                  ctypes.c_size_t(ws_bytes), _lib.stream_ptr())
        _lib.check(rc, "wv_dwt2d_forward")
    return out


def rawstack(x, copies=4, channels_last=False):
    """[B,C,H,W] -> [B,C,copies,H,W] identical planes (RawStackTransform, :172-188)."""
    lib = _lib.require_gpu()
    x, layout, B, C, H, W = _batch(x, channels_last, "rawstack", True, "")
    out = torch.empty((B, C, copies, H, W), dtype=torch.float32, device=x.device)
    if B == 0:
        return out
    with torch.cuda.device(x.device):
        rc = lib.wv_rawstack_forward(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), _lib.WV_DT_F32,
                                     B, C, H, W, copies, _lib.stream_ptr())
        _lib.check(rc, "wv_rawstack_forward")
    return out


def _lift_args(x, channels_last, mean, std, basis, levels, ll_only, what, on_gpu, note):
    """-> (x contiguous, C-ABI arguments between `in` and `out`, output shape).  The argument check is the library's."""
    x, layout, B, C, H, W = _batch(x, channels_last, what, on_gpu, note)
    if basis not in LIFT_BASIS:
        raise ValueError(f"{what}: basis must be 'haar' or 'cdf97', got {basis!r}")
    dt = _in_dtype(x)
    if (mean is None) != (std is None):
        raise ValueError(f"{what}: mean and std come together")
    if mean is not None and (len(mean) != C or len(std) != C):
        raise ValueError(f"{what}: mean / std need one value per channel ({C}), got {len(mean)} / {len(std)}")
    lib = _lib.load()
    b, levels, ll_only = LIFT_BASIS[basis], int(levels), int(bool(ll_only))
    _lib.check(lib.wv_lift_images_check(dt, layout, B, C, H, W, b, levels, ll_only), "wv_lift_images_check")
    h, w = (lib.wv_lift_out_size(H, b, levels), lib.wv_lift_out_size(W, b, levels)) if levels else (H, W)
    shape = (B, C, h, w) if levels == 0 or ll_only else (B, C, 4, h, w)
    fm = _lib.host_floats(mean) if mean is not None else None
    fs = _lib.host_floats(std) if std is not None else None
    args = (dt, layout, B, C, H, W, int(dt == _lib.WV_DT_U8), fm, fs, b, levels, ll_only)
    return x, args, shape


def lift_images(x, mean=None, std=None, basis="haar", levels=1, ll_only=False, channels_last=False):
    """The tensor tail of the legacy configs on a GPU batch: ToTensor -> [Normalize(mean, std)] -> [CustomTransform(levels,
    basis, coarse_only=True, ll_only)], bit-identical to the reference's float32 torch ops (wv_lift_images: one launch per
    level).  x: uint8 [B,C,H,W] (or [B,H,W,C] with channels_last: what size_images returns), divided by 255 and normalised;
    or float32, used as it is (mean / std must be None).  -> float32 [B,C,4,h,w] = (LL, LH, HL, HH) of the coarsest level,
    [B,C,h,w] with ll_only, [B,C,H,W] for levels = 0 (the conversion alone)."""
    lib = _lib.require_gpu()
    x, args, shape = _lift_args(x, channels_last, mean, std, basis, levels, ll_only, "lift_images", True,
                                " (lift_images_host is the host twin)")
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if shape[0] == 0:
        return out
    ws_bytes = lib.wv_lift_images_workspace_bytes(*args[2:6], args[9], args[10])
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.wv_lift_images(_lib.ptr(x), *args, _lib.ptr(out), _lib.ptr(ws), ctypes.c_size_t(ws_bytes), _lib.stream_ptr()),
                   "wv_lift_images")
    return out


def lift_images_host(x, mean=None, std=None, basis="haar", levels=1, ll_only=False, channels_last=False):
    """Host twin of lift_images (wv_lift_images_cpu): host tensors in, the same bits out."""
    lib = _lib.load()
    x, args, shape = _lift_args(x, channels_last, mean, std, basis, levels, ll_only, "lift_images_host", False,
                                "lift_images is the device function")
    out = torch.empty(shape, dtype=torch.float32)
    if shape[0] == 0:
        return out
    _lib.check(lib.wv_lift_images_cpu(_lib.ptr(x), *args, _lib.ptr(out)), "wv_lift_images_cpu")
    return out


# ---------------------------------------------------------------------------------------------------------------
# Host twins (wv_*_forward_cpu): what the plugins' __call__ runs inside forked DataLoader workers, where the
# reference runs pywt (flikr_coco.py:59-60 -> custom_transforms.py:145-157) and the GPU is out of reach.
# Host tensors in, host tensors out; single-threaded native code, no HIP call.
def swt2d_host(x, wavelet="haar", level=1, channels_last=False):
    """Host twin of swt2d: [B,C,H,W] (or [B,H,W,C]) uint8 / float32 on the CPU -> float32 [B,C,4,H,W]."""
    lib = _lib.load()
    x, layout, B, C, H, W = _batch(x, channels_last, "swt2d_host", False, _HOST_NOTE)
    lo, hi = get_filters(wavelet)
    out = torch.empty((B, C, 4, H, W), dtype=torch.float32)
    if B == 0:
        return out
    _swt_size(H, W, level)
    rc = lib.wv_swt2d_forward_cpu(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), B, C, H, W, level,
                                  _lib.host_floats(lo), _lib.host_floats(hi), len(lo))
    _lib.check(rc, "wv_swt2d_forward_cpu")
    return out


def swt2d_band_host(x, wavelet="haar", level=1, band=0, channels_last=False):
    """Host twin of swt2d_band (wv_swt2d_band_forward_cpu) -> float32 [B,C,H,W], bit-identical to
    ``swt2d_host(...)[:, :, band]``."""
    lib = _lib.load()
    x, layout, B, C, H, W = _batch(x, channels_last, "swt2d_band_host", False, _HOST_NOTE)
    lo, hi = get_filters(wavelet)
    band = int(band)
    if not 0 <= band <= 3:
        raise ValueError(f"swt2d_band_host: band must be 0..3 (cA, cH, cV, cD), got {band}")
    out = torch.empty((B, C, H, W), dtype=torch.float32)
    if B == 0:
        return out
    _swt_size(H, W, level)
    rc = lib.wv_swt2d_band_forward_cpu(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), band, B, C, H, W, level,
                                       _lib.host_floats(lo), _lib.host_floats(hi), len(lo))
    _lib.check(rc, "wv_swt2d_band_forward_cpu")
    return out


def dwt2d_host(x, wavelet="haar", level=1, channels_last=False):
    """Host twin of dwt2d -> float32 [B,C,4,H',W']."""
    lib = _lib.load()
    x, layout, B, C, H, W = _batch(x, channels_last, "dwt2d_host", False, _HOST_NOTE)
    lo, hi = get_filters(wavelet)
    Hn, Wn = lib.wv_dwt_out_len(H, len(lo), level), lib.wv_dwt_out_len(W, len(lo), level)
    out = torch.empty((B, C, 4, Hn, Wn), dtype=torch.float32)
    if B == 0:
        return out
    rc = lib.wv_dwt2d_forward_cpu(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), B, C, H, W, level,
                                  _lib.host_floats(lo), _lib.host_floats(hi), len(lo))
    _lib.check(rc, "wv_dwt2d_forward_cpu")
    return out


def rawstack_host(x, copies=4, channels_last=False):
    """Host twin of rawstack -> float32 [B,C,copies,H,W]."""
    lib = _lib.load()
    x, layout, B, C, H, W = _batch(x, channels_last, "rawstack_host", False, _HOST_NOTE)
    out = torch.empty((B, C, copies, H, W), dtype=torch.float32)
    if B == 0:
        return out
    rc = lib.wv_rawstack_forward_cpu(_lib.ptr(x), _in_dtype(x), layout, _lib.ptr(out), B, C, H, W, copies)
    _lib.check(rc, "wv_rawstack_forward_cpu")
    return out
