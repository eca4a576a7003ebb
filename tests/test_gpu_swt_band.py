"""The single-band SWT kernel (wv_swt2d_band_forward / transforms.swt2d_band) on the GPU: every element equals the same
element of the four-band kernel's band bit for bit -- fp32 and bf16 output, uint8 and float32 input, both layouts, all four
bands -- on the smallest shapes the sliding kernel takes, on a persistent launch (every plane checked), inside a
sentinel-filled buffer, on the shapes that fall back to the slice, and against the host twin."""
import numpy as np
import pytest
import torch

import swt_schedule_cases as S
from wvhash.transforms import swt2d, swt2d_band, swt2d_band_host

pytestmark = pytest.mark.gpu

# (wavelet, level, H, W): db2 L3 at W = 40 (W % 16 != 0: strided producer loads) and W = 48 (coalesced producer loads of
# planar uint8, 4 taps); haar and db4 at W = 48 take the 2- and 8-tap pixel windows of the coalesced producer through the
# single-band stage; W = 256 is the widest row the kernel takes
SHAPES = [("haar", 1, 40, 40), ("haar", 3, 40, 40), ("db2", 3, 64, 40), ("db2", 3, 64, 48), ("db4", 1, 40, 40),
          ("bior4.4", 1, 40, 40), ("db2", 2, 40, 256), ("haar", 1, 40, 48), ("db4", 1, 40, 48)]
B, C = 3, 3


def _inputs(H, W, seed):
    x = torch.from_numpy(S.noise(B, C, H, W, seed).copy())
    f = x.float() / 255.0
    return {"u8_planar": (x.cuda(), False), "u8_nhwc": (x.permute(0, 2, 3, 1).contiguous().cuda(), True),
            "f32_planar": (f.cuda(), False), "f32_nhwc": (f.permute(0, 2, 3, 1).contiguous().cuda(), True)}


@pytest.mark.parametrize("wl,lev,H,W", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_band_equals_four_band_kernel(wl, lev, H, W, out_dtype):
    assert S.fits(wl, lev, H, W)
    for kind, (x, cl) in _inputs(H, W, S.seed_of(wl, lev, H, W, C)).items():
        full = swt2d(x, wl, lev, channels_last=cl, out_dtype=out_dtype)
        for band in range(4):
            got = swt2d_band(x, wl, lev, band, channels_last=cl, out_dtype=out_dtype)
            assert got.shape == (B, C, H, W) and got.dtype == out_dtype and got.is_contiguous()
            assert torch.equal(got, full[:, :, band]), (kind, band)


@pytest.mark.parametrize("wl,lev,H,W,rem", [("db2", 3, 64, 48, 5), ("haar", 1, 40, 40, 0)])
def test_persistent_launch_every_plane(wl, lev, H, W, rem):
    """More planes than workgroups.  slide_launch (csrc/swt_slide.hpp, the launch rule k_swt_band shares with k_swt_slide)
    starts min(planes, 2 * CUs) workgroups -- two per CU by the occupancy the kernel is compiled for, the LDS ring allowing more -- rounded down to a multiple of 8; B is the
    smallest batch with B % 8 == rem and 3 * B >= 2.3 * 2 * CUs, so every workgroup loops over two or three planes and
    (rem = 5) the XCDs own different numbers of images.  Every plane is compared."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nb = S.persistent_batch(cu, C, rem)
    assert nb * C > S.WGS_PER_CU * cu
    x = torch.from_numpy(S.noise(nb, C, H, W, 7).copy()).cuda()
    full = swt2d(x, wl, lev)
    for band in range(4):
        got = swt2d_band(x, wl, lev, band)
        bad = (got != full[:, :, band]).flatten(2).any(dim=2).flatten().nonzero().flatten().tolist()
        assert not bad, f"band {band}: " + S.describe(bad, nb, C, cu)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_writes_stay_inside_out(out_dtype):
    wl, lev, H, W = "db2", 3, 64, 48
    x = torch.from_numpy(S.noise(B, C, H, W, 3).copy()).cuda()
    n, pad = B * C * H * W, 4096
    buf = torch.full((n + 2 * pad,), -7.0, dtype=out_dtype, device="cuda")
    out = buf[pad:pad + n].view(B, C, H, W)
    for band in range(4):
        got = swt2d_band(x, wl, lev, band, out_dtype=out_dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got, swt2d(x, wl, lev, out_dtype=out_dtype)[:, :, band])
        assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + n:] == -7.0).all())


def test_shapes_outside_the_sliding_kernel_are_sliced():
    x = torch.from_numpy(S.noise(2, 3, 40, 30, 5).copy()).cuda()          # W = 30: W % 4 != 0
    assert not S.fits("haar", 1, 40, 30)
    for band in range(4):
        assert torch.equal(swt2d_band(x, "haar", 1, band), swt2d(x, "haar", 1)[:, :, band])
    y = torch.from_numpy(S.noise(2, 3, 48, 48, 6).copy()).cuda()          # 6 taps: no sliding instantiation
    full = swt2d(y, "db3", 1, out_dtype=torch.bfloat16)
    for band in range(4):
        got = swt2d_band(y, "db3", 1, band, out_dtype=torch.bfloat16)
        assert got.is_contiguous() and torch.equal(got, full[:, :, band])


def test_arguments():
    x = torch.zeros(1, 3, 40, 40, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        swt2d_band(x, "haar", 1, 4)
    with pytest.raises(ValueError):
        swt2d_band(x, "haar", 4, 0)                                       # 40 is not a multiple of 16
    with pytest.raises(ValueError):
        swt2d_band(x, "haar", 1, 0, out=torch.empty(1, 3, 4, 40, 40, device="cuda"))
    assert swt2d_band(x[:0], "haar", 1, 2).shape == (0, 3, 40, 40)


def test_host_twin_equals_kernel():
    wl, lev, H, W = "db2", 3, 64, 48
    x = torch.from_numpy(S.noise(B, C, H, W, 9).copy())
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    for band in range(4):
        assert torch.equal(swt2d_band(x.cuda(), wl, lev, band).cpu(), swt2d_band_host(x, wl, lev, band))
        assert torch.equal(swt2d_band(nhwc.cuda(), wl, lev, band, channels_last=True).cpu(),
                           swt2d_band_host(nhwc, wl, lev, band, channels_last=True))
