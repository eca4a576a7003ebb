"""The single-band SWT on the host (no GPU): wv_swt2d_band_forward_cpu equals the matching band of wv_swt2d_forward_cpu bit
for bit, matches the oracle, and both new entry points check their arguments before touching anything."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import swt_np
from wvhash import _lib
from wvhash.transforms import get_filters, swt2d_band_host, swt2d_host

CONFIGS = [("haar", 1), ("haar", 2), ("haar", 3), ("db2", 1), ("db2", 3), ("db4", 1), ("bior4.4", 1)]
SHAPES = [(16, 24), (40, 56)]
B = 2


def _forms(H, W, seed):
    x = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B, 3, H, W), dtype=np.uint8))
    f = x.float() / 255.0
    return {"u8_nchw": (x, False), "u8_nhwc": (x.permute(0, 2, 3, 1).contiguous(), True),
            "f32_nchw": (f, False), "f32_nhwc": (f.permute(0, 2, 3, 1).contiguous(), True)}


@pytest.mark.parametrize("wl,lev", CONFIGS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_band_twin_equals_band_of_four_band_twin(wl, lev, H, W):
    for kind, (x, cl) in _forms(H, W, 31 * H + W + lev).items():
        full = swt2d_host(x, wl, lev, channels_last=cl)
        for band in range(4):
            got = swt2d_band_host(x, wl, lev, band, channels_last=cl)
            assert got.shape == (B, 3, H, W) and got.dtype == torch.float32
            assert torch.equal(got, full[:, :, band]), (kind, band)


def test_band_twin_matches_oracle():
    """The bound tests/test_gpu_swt.py holds the four-band kernel to: 4e-6 * 2^level (fused against separate multiply-add)."""
    wl, lev = "db2", 3
    img = np.random.default_rng(5).integers(0, 256, size=(B, 40, 56, 3), dtype=np.uint8)
    ref = swt_np.c_transform_batch(img, wl, lev)                                   # [B, 3, 4, H, W]
    for band in range(4):
        got = swt2d_band_host(torch.from_numpy(img), wl, lev, band, channels_last=True).numpy()
        assert np.abs(got - ref[:, :, band]).max() <= 4e-6 * 2 ** lev


def test_wrapper_arguments():
    x = torch.zeros(1, 3, 16, 24, dtype=torch.uint8)
    for band in (-1, 4):
        with pytest.raises(ValueError, match="band"):
            swt2d_band_host(x, "haar", 1, band)
    with pytest.raises(ValueError):
        swt2d_band_host(x, "haar", 4, 0)                                           # 24 is not a multiple of 16
    assert swt2d_band_host(x[:0], "haar", 1, 1).shape == (0, 3, 16, 24)


def test_entry_points_check_arguments_first():
    """Never-dereferenced pointers: every refusal happens on the host, before any access."""
    lib = _lib.load()
    one = ctypes.c_void_p(1)
    lo, hi = get_filters("db2")
    flo, fhi = _lib.host_floats(lo), _lib.host_floats(hi)
    for band in (-1, 4):
        rc = lib.wv_swt2d_band_forward(one, _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, one, _lib.WV_DT_F32, band, 1, 3, 64, 64, 3,
                                       flo, fhi, 4, None)
        assert rc == -22 and f"band {band}".encode() in lib.wv_last_error()
        rc = lib.wv_swt2d_band_forward_cpu(one, _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, one, band, 1, 3, 64, 64, 3, flo, fhi, 4)
        assert rc == -22 and f"band {band}".encode() in lib.wv_last_error()
    text = b"swt: H=60, W=64 must be multiples of 2^level=8 (PyWavelets raises ValueError here)"
    rc = lib.wv_swt2d_band_forward(one, _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, one, _lib.WV_DT_F32, 0, 1, 3, 60, 64, 3, flo, fhi,
                                   4, None)
    assert rc == -22 and lib.wv_last_error() == text
    rc = lib.wv_swt2d_band_forward_cpu(one, _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, one, 0, 1, 3, 60, 64, 3, flo, fhi, 4)
    assert rc == -22 and lib.wv_last_error() == text
    # the four-band entry point's own text for the same mistake
    assert lib.wv_swt2d_forward(one, 0, 0, one, 1, 1, 3, 60, 64, 3, flo, fhi, 4, None, 0, None) == -22
    assert lib.wv_last_error() == text
    # a shape outside the sliding kernel: the planner's sentence, nothing launched
    rc = lib.wv_swt2d_band_forward(one, _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, one, _lib.WV_DT_F32, 0, 1, 3, 48, 64, 3, flo, fhi,
                                   4, None)
    assert rc == _lib.WV_ENOTSUP == -95 and b"H >= 58" in lib.wv_last_error()


def test_header_declares_both_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "wvhash.h")).read()
    assert "int wv_swt2d_band_forward(" in text and "int wv_swt2d_band_forward_cpu(" in text
    assert "wv_swt2d_band_forward" in _lib.SIGNATURES and "wv_swt2d_band_forward_cpu" in _lib.SIGNATURES


def test_plugin_apply_band_on_host_tensors():
    """Host tensors through the plugins take the host twins: SWTTransform the single-band twin, the others transform and slice."""
    from wvhash.transforms import RawStackTransform, SWTTransform, rawstack_host
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(2, 3, 40, 40), dtype=np.uint8))
    for band in range(4):
        got = SWTTransform(1, "haar", defer=True).apply_band(x, band)
        assert got.is_contiguous() and torch.equal(got, swt2d_host(x, "haar", 1)[:, :, band])
        nhwc = SWTTransform(1, "haar", defer=True).apply_band(x.permute(0, 2, 3, 1).contiguous(), band, channels_last=True)
        assert torch.equal(nhwc, got)
        raw = RawStackTransform(copies=4, defer=True).apply_band(x, band)
        assert raw.is_contiguous() and torch.equal(raw, rawstack_host(x, 4)[:, :, band])
    assert SWTTransform(1, "haar", defer=True).apply_band(x, 1, out_dtype=torch.bfloat16).dtype == torch.bfloat16


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_device_function_fails_loudly_without_gpu():
    from wvhash.transforms import swt2d_band
    with pytest.raises(_lib.WvhashUnavailable):
        swt2d_band(torch.zeros(1, 3, 40, 40, dtype=torch.uint8), "haar", 1, 2)
