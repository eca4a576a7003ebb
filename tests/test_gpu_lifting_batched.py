"""GPU: the batched tensor tail (wv_lift_images) against its host twin, bit for bit, and the deferred pipelines end to end.
The twin itself is pinned to live torch ops and the reference-made lifting vectors by tests/test_host_lifting.py."""
import ctypes

import numpy as np
import pytest
import torch

import lifting_cases as LC
from wvhash import _lib

pytestmark = pytest.mark.gpu
NCHW, NHWC = _lib.WV_LAYOUT_NCHW, _lib.WV_LAYOUT_NHWC
GUARD = 256                                   # fp32 words of NaN on each side of `out` and of the workspace
NAN_BITS = np.float32(np.nan).view(np.int32)


def run_gpu(lib, x, layout, B, C, H, W, mean, std, basis, levels, ll_only, ws_bytes=None):
    """wv_lift_images with `out` and the workspace inside one NaN-filled buffer -> (rc, out, guards untouched)."""
    shape = LC.out_shape(lib, B, C, H, W, basis, levels, ll_only)
    n_out = int(np.prod(shape))
    need = lib.wv_lift_images_workspace_bytes(B, C, H, W, LC.BASES.index(basis), levels)
    assert need % 4 == 0
    n_ws = need // 4
    big = torch.full((3 * GUARD + n_out + n_ws,), float("nan"), dtype=torch.float32, device="cuda")
    out, ws = big[GUARD:GUARD + n_out], big[2 * GUARD + n_out:2 * GUARD + n_out + n_ws]
    dt = _lib.WV_DT_U8 if x.dtype == torch.uint8 else _lib.WV_DT_F32
    rc = lib.wv_lift_images(_lib.ptr(x), dt, layout, B, C, H, W, int(dt == _lib.WV_DT_U8), LC.floats(mean), LC.floats(std),
                            LC.BASES.index(basis), levels, int(ll_only), _lib.ptr(out), ctypes.c_void_p(ws.data_ptr() if n_ws else 0),
                            ctypes.c_size_t(need if ws_bytes is None else ws_bytes), _lib.stream_ptr())
    host = big.cpu().numpy().view(np.int32)
    guards = np.concatenate([host[:GUARD], host[GUARD + n_out:2 * GUARD + n_out], host[2 * GUARD + n_out + n_ws:]])
    return rc, host[GUARD:GUARD + n_out].view(np.float32).reshape(shape), bool((guards == NAN_BITS).all())


def edge_sizes(tile):
    """Sizes that end two samples before, exactly at, two past and four past one tile and two tiles."""
    return [k * tile + d for k in (1, 2) for d in (-2, 0, 2, 4)]


def shapes(lib):
    th, tw = lib.wv_lift_images_tile(0), lib.wv_lift_images_tile(1)
    assert th >= 4 and tw >= 4
    s = LC.SMALL
    small = [(s[i], s[(i + k) % len(s)]) for k in (0, 5) for i in range(len(s))]
    small += [(100, 75), (75, 100), (50, 30), (30, 50)]          # turn odd inside the cascade (haar at 3 levels, cdf 9/7 at 2)
    edges = list(zip(edge_sizes(th), edge_sizes(tw))) + [(edge_sizes(th)[-1], 5), (7, edge_sizes(tw)[-1])]
    return small + edges


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("basis", LC.BASES)
def test_kernel_equals_the_twin_bit_for_bit(basis, dtype):
    lib = _lib.require_gpu()
    rng = np.random.default_rng(17)
    B, C = 3, 3
    mean, std = LC.UNEQUAL if dtype == "uint8" else (None, None)
    for n, (H, W) in enumerate(shapes(lib)):
        if dtype == "uint8":
            x = rng.integers(0, 256, (B, C, H, W), dtype=np.uint8)
        else:
            x = rng.standard_normal((B, C, H, W)).astype(np.float32)
            x[0, 0, 0, 0] = -0.0
        for layout in (NCHW, NHWC):
            src = LC.nhwc(x) if layout == NHWC else x
            dev = torch.from_numpy(src).cuda()
            for levels in (1, 2, 3):
                for ll_only in (0, 1):
                    rc, want = LC.run_cpu(lib, src, layout, B, C, H, W, mean, std, basis, levels, ll_only)
                    assert rc == 0, lib.wv_last_error()
                    rc, got, clean = run_gpu(lib, dev, layout, B, C, H, W, mean, std, basis, levels, ll_only)
                    assert rc == 0, lib.wv_last_error()
                    assert LC.same_bits(got, want), (H, W, layout, levels, ll_only)        # no NaN left: every element written
                    assert clean, (H, W, layout, levels, ll_only)


def test_conversion_alone_and_every_byte_value():
    lib = _lib.require_gpu()
    rng = np.random.default_rng(5)
    x = np.stack([rng.permutation(np.arange(270) % 256).astype(np.uint8).reshape(18, 15) for _ in range(3)])[None]
    for mean, std in ((None, None), LC.IMAGENET, LC.UNEQUAL):
        want = LC.to_tensor_normalize(x, mean, std).numpy()
        for layout in (NCHW, NHWC):
            src = LC.nhwc(x) if layout == NHWC else x
            rc, got, clean = run_gpu(lib, torch.from_numpy(src).cuda(), layout, 1, 3, 18, 15, mean, std, "haar", 0, 0)
            assert rc == 0 and clean and LC.same_bits(got, want), (mean, layout)           # the live torch ops themselves
            for basis in LC.BASES:
                rc, got, clean = run_gpu(lib, torch.from_numpy(src).cuda(), layout, 1, 3, 18, 15, mean, std, basis, 2, 0)
                assert rc == 0 and clean and LC.same_bits(got, LC.expected(want, basis, 2, 0)), (mean, layout, basis)


@pytest.mark.parametrize("side,basis,levels", [(224, "haar", 1), (224, "haar", 3), (448, "cdf97", 1)])
def test_pipeline_shapes(side, basis, levels):
    """What cub_dwt, a three-level haar cascade and cub_dwt_cdf97 run: the sized uint8 NHWC batch, ImageNet constants."""
    from wvhash.transforms import lift_images, lift_images_host
    x = torch.from_numpy(np.random.default_rng(side + levels).integers(0, 256, (2, side, side, 3), dtype=np.uint8))
    want = lift_images_host(x, *LC.IMAGENET, basis=basis, levels=levels, channels_last=True)
    got = lift_images(x.cuda(), *LC.IMAGENET, basis=basis, levels=levels, channels_last=True)
    h = side >> levels
    assert tuple(got.shape) == (2, 3, 4, h, h) and got.is_cuda and LC.same_bits(got, want)
    again = lift_images(x.cuda(), *LC.IMAGENET, basis=basis, levels=levels, channels_last=True)
    assert LC.same_bits(again, got)                                                        # a repeat run: identical bits
    oracle = LC.expected(LC.to_tensor_normalize(x.permute(0, 3, 1, 2), *LC.IMAGENET).numpy(), basis, levels, 0)
    assert LC.same_bits(got, oracle)


def test_deferred_pipelines_end_to_end():
    """Five images of different sizes through the cub_dwt train node (two sizing stages + jitter + tail): GPU = host-twin
    pipeline = PIL + torch + oracle; the basic train node gives the plain float batch."""
    from wvhash.transforms import build_transform, find_wavelet_transform, raw_collate
    images = LC.pil_images(5, seed=31)
    for node, shape in ((LC.CUB_DWT["train"], (5, 3, 4, 112, 112)), (LC.BASIC["train"], (5, 3, 224, 224))):
        torch.manual_seed(123)
        deferred = build_transform(node, defer=True, sizing="device")
        batch = raw_collate([deferred(img) for img in images])
        plugin = find_wavelet_transform(deferred)
        on_host = plugin.apply_batch(batch)
        on_gpu = plugin.apply_batch(batch.cuda())
        assert on_gpu.is_cuda and tuple(on_gpu.shape) == shape and on_gpu.dtype == torch.float32
        assert LC.same_bits(on_gpu, on_host)
        torch.manual_seed(123)
        front = build_transform({k: v for k, v in node.items() if k != "CustomTransform"})      # PIL + torch, per image
        t = torch.stack([front(img) for img in images]).numpy()
        levels = node.get("CustomTransform", {}).get("decompose_levels", 0)
        assert LC.same_bits(on_gpu, LC.expected(t, "haar", levels, 0))


def test_too_small_workspace_is_refused_before_any_launch():
    lib = _lib.require_gpu()
    x = torch.zeros((2, 3, 32, 32), dtype=torch.uint8, device="cuda")
    need = lib.wv_lift_images_workspace_bytes(2, 3, 32, 32, 0, 3)
    assert need > 0
    rc, got, clean = run_gpu(lib, x, NCHW, 2, 3, 32, 32, None, None, "haar", 3, 0, ws_bytes=need - 1)
    assert rc == -12 and b"workspace_bytes" in lib.wv_last_error()
    assert clean and (got.view(np.int32) == NAN_BITS).all()                                # nothing ran
