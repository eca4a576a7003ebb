"""The plane schedule of the sliding SWT kernel (csrc/swt_slide.hip; PlaneSchedule, csrc/swt_slide.hpp): every plane of a
launch, not a sample of them.

slide_launch (csrc/swt_slide.hpp) starts min(planes, 2 * CUs) workgroups.  With more planes than that a workgroup loops
over several planes of its XCD and reuses the LDS ring, the producer's prefetch and the barrier pairing from one plane to the next; with a plane
count that is a multiple of 8 the images are dealt to the 8 XCDs even when those own unequal numbers of them or none.  The
batches here (tests/swt_schedule_cases.py, checked without a GPU by tests/test_swt_schedule_cases.py) give every workgroup
two or three planes with unequal XCD shares, at heights of both parities of the chunk count, for every (taps, level) the
kernel is built for, every input form it reads (planar uint8 aligned and not, interleaved uint8, planar and interleaved
float32), C = 1, 3, 4, 8 and both output types.

Every case: the output buffers are pre-filled with NaN (a plane nobody wrote cannot pass on what the allocator left there);
the reference-layout result comes from swt2d, the band-major one from wv_swt2d_forward_ex directly, which only the sliding
kernel serves (return code 0 = the sliding kernel took the shape); both are finite, every plane is within 4e-6 * 2^level of
the C oracle (the bound of tests/test_gpu_swt.py), and the bits equal those of the same images transformed one per call,
where one workgroup computes one plane: what a plane holds does not depend on who computed it or when.
"""
import ctypes

import numpy as np
import pytest
import torch

import swt_schedule_cases as sc
from wvhash import _lib
from wvhash.transforms import get_filters, swt2d

pytestmark = pytest.mark.gpu

TORCH_DT = {torch.float32: _lib.WV_DT_F32, torch.bfloat16: _lib.WV_DT_BF16}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def nan_buffer(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def forward_ex(x, channels_last, wl, lev, out_ptr, out_dtype, band_stride):
    """wv_swt2d_forward_ex, band-major, on the whole of `x` -> return code."""
    lib = _lib.require_gpu()
    if channels_last:
        B, H, W, C = x.shape
    else:
        B, C, H, W = x.shape
    lo, hi = get_filters(wl)
    in_dt = _lib.WV_DT_U8 if x.dtype == torch.uint8 else _lib.WV_DT_F32
    layout = _lib.WV_LAYOUT_NHWC if channels_last else _lib.WV_LAYOUT_NCHW
    assert x.is_contiguous()                     # no workspace: the sliding kernel, the only one behind this call, has none
    return lib.wv_swt2d_forward_ex(_lib.ptr(x), in_dt, layout, ctypes.c_void_p(out_ptr), TORCH_DT[out_dtype],
                                   _lib.WV_BANDS_OUTER, band_stride, B, C, H, W, lev, _lib.host_floats(lo),
                                   _lib.host_floats(hi), len(lo), None, ctypes.c_size_t(0), _lib.stream_ptr())


def band_major(x, channels_last, wl, lev, shape, out_dtype=torch.float32):
    """[4, B, C, H, W] from one direct call into a NaN-filled buffer; the sliding kernel must have taken it."""
    out = nan_buffer((4,) + shape, out_dtype)
    rc = forward_ex(x, channels_last, wl, lev, out.data_ptr(), out_dtype, out[0].numel())
    assert rc == 0, (rc, _lib.load().wv_last_error())
    return out


def one_per_call(x, channels_last, wl, lev, shape, out_dtype=torch.float32):
    """[B, C, 4, H, W] from launches of one workgroup per plane: one image per call, or one plane per call where the
    image's own plane count would switch the XCD mapping on (C % 8 == 0; planar input only)."""
    B, C = shape[:2]
    out = nan_buffer((B, C, 4) + shape[2:], out_dtype)
    for b in range(B):
        if C % 8:
            swt2d(x[b:b + 1], wl, lev, channels_last=channels_last, out_dtype=out_dtype, out=out[b:b + 1])
        else:
            assert not channels_last
            for c in range(C):
                swt2d(x[b:b + 1, c:c + 1], wl, lev, out_dtype=out_dtype, out=out[b:b + 1, c:c + 1])
    return out


def planes_that_differ(a, b):
    """Flat plane numbers (b * C + c) at which two [B, C, 4, H, W] tensors do not hold the same bits."""
    same = (a.view(torch.int32 if a.dtype == torch.float32 else torch.int16) ==
            b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)).flatten(2).all(dim=2)
    return torch.nonzero(~same.flatten()).flatten().tolist()


def check_case(wl, lev, H, W, B, C, kind, out_dtype=torch.float32):
    """All the checks of the module docstring on one batch -> the checked fp32 (or bf16) reference-layout result."""
    seed = sc.seed_of(wl, lev, H, W, C)
    xh = sc.noise(B, C, H, W, seed)
    x, cl = sc.device_input(xh, kind)
    shape = (B, C, H, W)
    got = swt2d(x, wl, lev, channels_last=cl, out_dtype=out_dtype, out=nan_buffer((B, C, 4, H, W), out_dtype))
    outer = band_major(x, cl, wl, lev, shape, out_dtype)
    single = one_per_call(x, cl, wl, lev, shape, out_dtype)
    torch.cuda.synchronize()
    where = lambda bad: sc.describe(bad, B, C, cus())
    unwritten = torch.nonzero(~torch.isfinite(got).flatten(2).all(dim=2).flatten()).flatten().tolist()
    assert not unwritten, "planes with values that are not finite (never written?): " + where(unwritten)
    assert torch.isfinite(outer).all() and torch.isfinite(single).all()
    if out_dtype == torch.float32:
        ref = torch.from_numpy(sc.reference(wl, lev, B, C, H, W, seed)).cuda()
        err = (got - ref).abs().flatten(2).amax(dim=2).flatten()
        worst = int(err.argmax())
        print(f"{wl} L{lev} {H}x{W} B={B} C={C} {kind}: max |hip - oracle| = {float(err[worst]):.3e} (bound {sc.tol(lev):.3e})")
        assert float(err[worst]) <= sc.tol(lev), f"worst plane off by {float(err[worst]):.3e}: " + where([worst])
    bad = planes_that_differ(got, single)
    assert not bad, "planes whose bits differ from the one-image-per-call result: " + where(bad)
    bad = planes_that_differ(outer.permute(1, 2, 0, 3, 4), got)
    assert not bad, "band-major planes that differ from the reference layout: " + where(bad)
    return got, x, cl


# ------------------------------------------------------------------------------------------------ a, b: persistent launches
@pytest.mark.parametrize("wl,lev,H,W,C,rem,kind", sc.flat(sc.SHIPPED_CASES + sc.OTHER_CASES))
def test_persistent_launch_every_plane(wl, lev, H, W, C, rem, kind):
    B = sc.persistent_batch(cus(), C, rem)
    grid, nxcd, wg, it = sc.schedule(B, C, cus())
    per_wg = np.bincount(wg.ravel(), minlength=grid)
    assert grid < B * C and nxcd == 8 and B % 8 == rem and 2 <= per_wg.min() and per_wg.max() <= 3
    check_case(wl, lev, H, W, B, C, kind)


@pytest.mark.parametrize("kind", sc.BF16_KINDS)
@pytest.mark.parametrize("wl,lev,H,W,C,rem", sc.BF16_CASES)
def test_persistent_launch_bf16_is_rounded_fp32(wl, lev, H, W, C, rem, kind):
    B = sc.persistent_batch(cus(), C, rem)
    b16, x, cl = check_case(wl, lev, H, W, B, C, kind, out_dtype=torch.bfloat16)
    f32 = swt2d(x, wl, lev, channels_last=cl, out=nan_buffer((B, C, 4, H, W)))
    ref = torch.from_numpy(sc.reference(wl, lev, B, C, H, W, sc.seed_of(wl, lev, H, W, C))).cuda()
    assert float((f32 - ref).abs().max()) <= sc.tol(lev)
    bad = planes_that_differ(b16, f32.to(torch.bfloat16))
    assert b16.dtype == torch.bfloat16 and not bad, "bf16 planes that are not the rounded fp32 planes: " + sc.describe(bad, B, C, cus())


# ------------------------------------------------------------------------------------------------ c: few planes, XCD mapping
@pytest.mark.parametrize("B,C", list(sc.FEW_PLANES))
@pytest.mark.parametrize("wl,lev,H,W", sc.FEW_SHAPES)
def test_xcd_mapping_with_few_planes(wl, lev, H, W, B, C):
    grid, nxcd, _, _ = sc.schedule(B, C, cus())
    assert grid == B * C and nxcd == sc.FEW_PLANES[(B, C)]
    check_case(wl, lev, H, W, B, C, "u8_planar")


# ------------------------------------------------------------------------------------------------ d: padded, shared buffer
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wl,lev,H,W", sc.FEW_SHAPES)
def test_band_major_chunks_into_one_padded_buffer(wl, lev, H, W, out_dtype):
    """What swt2d's chunk loop does past 65,535 images, at 3 + 5: each call gets the whole buffer's band stride and its own
    batch; here the stride also leaves 64 elements between the bands, which must stay untouched."""
    B, b0, C, pad = sc.SPLIT_B, sc.SPLIT_B0, sc.SPLIT_C, sc.SPLIT_PAD
    seed = sc.seed_of(wl, lev, H, W, C)
    x, cl = sc.device_input(sc.noise(B, C, H, W, seed), "u8_planar")
    n = B * C * H * W
    stride = n + pad
    flat = nan_buffer((4 * stride,), out_dtype)
    size = flat.element_size()
    for lo_b, hi_b in ((0, b0), (b0, B)):
        rc = forward_ex(x[lo_b:hi_b], cl, wl, lev, flat.data_ptr() + lo_b * C * H * W * size, out_dtype, stride)
        assert rc == 0, (rc, _lib.load().wv_last_error())
    whole = band_major(x, cl, wl, lev, (B, C, H, W), out_dtype)
    torch.cuda.synchronize()
    rows = flat.view(4, stride)
    assert torch.isnan(rows[:, n:]).all(), "the padding after a band was written"
    bands = rows[:, :n].reshape(4, B, C, H, W)
    bad = planes_that_differ(bands.permute(1, 2, 0, 3, 4), whole.permute(1, 2, 0, 3, 4))
    assert not bad, "planes of the two-call buffer that differ from the one-call result: " + sc.describe(bad, B, C, cus())
    assert torch.isfinite(bands).all() and torch.isfinite(whole).all()
    ref = torch.from_numpy(sc.reference(wl, lev, B, C, H, W, seed)).cuda().permute(2, 0, 1, 3, 4)
    # fp32 value g within tol of the oracle; bf16 rounds it to nearest with 8 significant bits: |bf16(g) - g| <= 2^-8 |g|
    slack = 0.0 if out_dtype == torch.float32 else 2.0 ** -8
    assert bool(((bands.float() - ref).abs() <= sc.tol(lev) + slack * (ref.abs() + sc.tol(lev))).all())
