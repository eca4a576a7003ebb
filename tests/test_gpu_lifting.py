"""GPU: the legacy lifting transforms (wv_lifting2d_forward, CustomTransform) against vectors produced by the
REFERENCE's own fast_haar_2d_op / fast_cdf97_2d_op (tests/golden/lifting_golden.npz) -- bit for bit."""
import os

import numpy as np
import pytest
import torch

from oracle import lifting_np

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lifting_golden.npz")


def test_lifting_kernel_is_bit_identical_to_the_reference():
    from wvhash.transforms import Cdf97Lifting, HaarLifting
    gold = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in gold.files})
    for name in names:
        basis = "haar" if name.startswith("haar") else "cdf97"
        shape, seed = tuple(gold[f"{name}/shape"]), int(gold[f"{name}/seed"])
        x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        levels = len([k for k in gold.files if k.startswith(name + "/l") and k.endswith("/ll")])
        mod = (HaarLifting if basis == "haar" else Cdf97Lifting)(n_levels=levels)
        approx, details = mod(x.cuda())
        for lev in range(levels):
            assert np.array_equal(approx[lev].cpu().numpy(), gold[f"{name}/l{lev}/ll"]), (name, lev, "ll")
            assert np.array_equal(details[lev].cpu().numpy(), gold[f"{name}/l{lev}/hi"]), (name, lev, "hi")


@pytest.mark.parametrize("basis,levels,shape", [("haar", 1, (3, 224, 224)), ("haar", 3, (2, 3, 100, 75)), ("cdf97", 1, (3, 448, 448)),
                                                ("cdf97", 2, (1, 3, 50, 30))])
def test_custom_transform_matches_oracle_and_keeps_the_callers_device(basis, levels, shape):
    from wvhash.transforms import CustomTransform
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    y = CustomTransform(decompose_levels=levels, basis=basis)(x)            # CPU in -> CPU out (worker-style call)
    assert not y.is_cuda
    ref = lifting_np.custom_transform(x.numpy(), levels, basis)
    assert y.shape == ref.shape and np.array_equal(y.numpy(), ref)
    ll = CustomTransform(decompose_levels=levels, basis=basis, ll_only=True)(x.cuda())
    assert ll.is_cuda and np.array_equal(ll.cpu().numpy(), lifting_np.custom_transform(x.numpy(), levels, basis, ll_only=True))


def test_custom_transform_equals_the_composition_of_the_lifting_modules():
    """CustomTransform's one batched call (wv_lift_images) returns the bits of the level cascade: zero pad, one
    wv_lifting2d_forward per level (HaarLifting / Cdf97Lifting), the coarsest approximation stacked on its details.  Both
    sides of both inputs are odd or no multiple of 4: every level pads."""
    from wvhash.transforms import Cdf97Lifting, CustomTransform, HaarLifting
    for basis, levels in [(b, n) for b in ("haar", "cdf97") for n in (1, 3)]:
        for seed, shape in enumerate([(2, 3, 37, 50), (3, 19, 26)]):
            x = torch.randn(shape, generator=torch.Generator().manual_seed(20 + seed))
            approx, details = (HaarLifting if basis == "haar" else Cdf97Lifting)(n_levels=levels)(x.cuda())
            full = CustomTransform(levels, basis)(x.cuda())
            ll = CustomTransform(levels, basis, ll_only=True)(x.cuda())
            assert full.is_cuda and torch.equal(full, torch.cat([approx[-1].unsqueeze(-3), details[-1]], -3)), (basis, levels, shape)
            assert ll.is_cuda and torch.equal(ll, approx[-1]), (basis, levels, shape)
            on_cpu = CustomTransform(levels, basis, device="cuda")(x)
            assert not on_cpu.is_cuda and torch.equal(on_cpu, full.cpu()), (basis, levels, shape)


def test_lifting_stride_loops_serve_what_the_capped_grid_leaves():
    """[9, 2048, 2048]: 9 * 1024 * 2048 = 18.9M pairs per pass against the 65536 x 256 = 16,777,216 threads k_lift_rows and
    k_lift_cols are capped at.  Planes 0..7 fill the first round exactly, so plane 8 is served by the second alone.  The
    first, the last of the first round and plane 8 against the oracle, bit for bit."""
    from wvhash.transforms import HaarLifting
    P, H, W = 9, 2048, 2048
    assert (P - 1) * (H // 2) * W == (1 << 16) * 256
    x = torch.randn((P, H, W), generator=torch.Generator().manual_seed(31))
    approx, details = HaarLifting(n_levels=1)(x.cuda())
    full = torch.cat([approx[-1].unsqueeze(-3), details[-1]], -3)
    assert full.is_cuda and tuple(full.shape) == (P, 4, H // 2, W // 2)
    for p in (0, 7, 8):
        ref = lifting_np.custom_transform(x[p].numpy(), 1, "haar")
        assert np.array_equal(full[p].cpu().numpy().view(np.int32), ref.view(np.int32)), p


def test_full_subbands_level1_and_errors_and_resize():
    from wvhash import _lib
    from wvhash.transforms import CustomTransform, ResizeSubBands
    x = torch.randn(3, 32, 48, generator=torch.Generator().manual_seed(6))
    y = CustomTransform(decompose_levels=1, basis="cdf97", coarse_only=False)(x)
    assert np.array_equal(y.numpy(), lifting_np.custom_transform(x.numpy(), 1, "cdf97", coarse_only=False))
    with pytest.raises(NotImplementedError):
        CustomTransform(decompose_levels=2, basis="haar", coarse_only=False)(x)
    r = ResizeSubBands(20)(y)                                                # [3, 4, 16, 24] -> shorter side 20
    assert tuple(r.shape) == (3, 4, 20, 30)
    ref = torch.nn.functional.interpolate(y.reshape(12, 1, 16, 24), size=(20, 30), mode="bilinear", align_corners=False, antialias=True)
    assert torch.equal(r, ref.reshape(3, 4, 20, 30))
    lib = _lib.require_gpu()
    t = torch.zeros(64, device="cuda")
    assert lib.wv_lifting2d_forward(_lib.ptr(t), 1, 7, 8, 0, _lib.ptr(t), _lib.ptr(t), None, 0, None) == -22   # odd H
    assert lib.wv_lifting2d_forward(_lib.ptr(t), 1, 8, 8, 0, _lib.ptr(t), _lib.ptr(t), None, 0, None) == -12   # no workspace
