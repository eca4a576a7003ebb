"""The sliding SWT kernel's coalesced row pass against its strided row pass, bit for bit.

Planar uint8 batches with W % 16 == 0 and a 16-byte aligned pointer take the coalesced producer: every lane loads its own
run of 16 pixels, converts each pixel once, computes outputs 0..15 of every level below the last and takes the values the
next level reads past them from the lane to its right (the row wraps onto itself).  The strided producer loads and filters
a run's whole window by itself.  It runs in the same build for the same pixels when the batch is interleaved
([B,H,W,3], channels_last=True) and when the planar batch starts at an address that is not a multiple of 16.  Both accumulate
each output's taps in the same order, so all three results must be equal (torch.equal), not merely close.

Shapes (B = 3, C = 3) reach every lane mapping of the coalesced producer: W = 48 (3 runs, 21 rows per wave capped at the 16
rows of a chunk, three idle waves), 64 (4 runs, 16 rows per wave), 224 (14 runs, 8 spare lanes per wave), 256 (16 runs, no
spare lanes).  H = 64 and H = 58: in both the last chunk of 16 rows is only partly consumed by the column cascade, so the
rows the producer no longer filters are exercised.  The transform rejects a height that is no multiple of 2^level (as
PyWavelets does), so H = 58 runs at level 1 only; at levels 2 and 3, H = 64 is the smallest height of the list that runs.
Every (wavelet, level) pair listed fits the sliding kernel's window at these sizes.
"""
import numpy as np
import pytest
import torch

from oracle import swt_np
from wvhash import synth
from wvhash.transforms import swt2d

pytestmark = pytest.mark.gpu

B, C, R = 3, 3, 16
WAVELETS = [("haar", 1), ("haar", 2), ("haar", 3), ("db2", 1), ("db2", 2), ("db2", 3), ("db4", 1), ("bior4.4", 1)]
CASES = [(wl, lev, H, W) for wl, lev in WAVELETS for H in (58, 64) for W in (48, 64, 224, 256) if H % (1 << lev) == 0]


def random_batch(H, W, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B, C, H, W), dtype=np.uint8))


def border_batch(H, W):
    """Nonzero pixels only in columns 0 and W-1 and rows 0 and H-1: what the periodic wrap of the hand-over carries."""
    x = torch.zeros(B, C, H, W, dtype=torch.uint8)
    ramp_w = (torch.arange(W) * 5 % 255 + 1).to(torch.uint8)
    ramp_h = (torch.arange(H) * 3 % 255 + 1).to(torch.uint8)
    for b in range(B):
        for c in range(C):
            x[b, c, 0, :] = torch.roll(ramp_w, b + c)
            x[b, c, H - 1, :] = torch.roll(ramp_w, 7 * b + c + 1)
            x[b, c, :, 0] = torch.roll(ramp_h, b + 2 * c)
            x[b, c, :, W - 1] = torch.roll(ramp_h, 3 * b + c + 2)
    return x


def run_constant_batch(H, W):
    """Every run of 16 columns holds one constant that differs from its neighbours' in the row and in the wave: a
    hand-over from the wrong lane changes the result."""
    nrun = W // R
    rows = torch.arange(H).view(1, 1, H, 1)
    runs = torch.arange(nrun).view(1, 1, 1, nrun)
    plane = torch.arange(B * C).view(B, C, 1, 1)
    val = ((rows * nrun + runs) * 37 + plane * 11) % 256
    return val.to(torch.uint8).repeat_interleave(R, dim=3).contiguous()


def coalesced(x, wl, lev, **kw):
    xg = x.cuda()
    assert xg.data_ptr() % 16 == 0 and xg.is_contiguous()
    return swt2d(xg, wl, lev, **kw)


def strided_interleaved(x, wl, lev):
    return swt2d(x.permute(0, 2, 3, 1).contiguous().cuda(), wl, lev, channels_last=True)


def strided_unaligned(x, wl, lev):
    n = x.numel()
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    view = buf[4:4 + n].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return swt2d(view, wl, lev)


@pytest.mark.parametrize("wl,lev,H,W", CASES)
def test_coalesced_row_pass_equals_strided_row_pass(wl, lev, H, W):
    batches = {"random": random_batch(H, W, seed=1000 * lev + H + W), "border": border_batch(H, W),
               "run constants": run_constant_batch(H, W)}
    for name, x in batches.items():
        got = coalesced(x, wl, lev)
        assert tuple(got.shape) == (B, C, 4, H, W) and torch.isfinite(got).all(), name
        assert torch.equal(got, strided_interleaved(x, wl, lev)), f"{name}: differs from the interleaved (strided) path"
        assert torch.equal(got, strided_unaligned(x, wl, lev)), f"{name}: differs from the unaligned (strided) path"


def test_db2_l3_224_against_the_oracle_and_bf16_is_rounded_fp32():
    img = synth.natural_images(B, 224, 224, seed=224 * 7 + 224 + 3)          # [B, H, W, 3]
    x = torch.from_numpy(img).permute(0, 3, 1, 2).contiguous()
    got = coalesced(x, "db2", 3)
    ref = swt_np.c_transform_batch(img, "db2", 3)
    assert np.abs(got.cpu().numpy() - ref).max() <= 4e-6 * 2 ** 3                # the bound of tests/test_gpu_swt.py
    b16 = coalesced(x, "db2", 3, out_dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16, got.to(torch.bfloat16))
