"""CPU: the host twin of the batched tensor tail (wv_lift_images_cpu), its argument check, and the Python layer that folds
ToTensor -> Normalize -> CustomTransform into one deferred plugin.  Comparisons are on bit patterns: -0.0 is not +0.0.
ToTensor / Normalize expectations are live torch ops; the lifting expectation is oracle.lifting_np (bit-pinned to the
reference by tests/golden/lifting_golden.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import lifting_cases as LC
from oracle import lifting_np
from wvhash import _lib

GOLD = os.path.join(os.path.dirname(__file__), "golden", "lifting_golden.npz")
NCHW, NHWC = _lib.WV_LAYOUT_NCHW, _lib.WV_LAYOUT_NHWC


def test_twin_reproduces_the_reference_made_vectors():
    from wvhash.transforms import lift_images_host
    gold = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in gold.files})
    assert len(names) == 8
    for name in names:
        basis = "haar" if name.startswith("haar") else "cdf97"
        shape, seed = tuple(gold[f"{name}/shape"]), int(gold[f"{name}/seed"])
        x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        planes = x.reshape(-1, 1, *shape[-2:])
        levels = len([k for k in gold.files if k.startswith(name + "/l") and k.endswith("/ll")])
        for lev in range(1, levels + 1):
            ll, hi = gold[f"{name}/l{lev - 1}/ll"], gold[f"{name}/l{lev - 1}/hi"]
            out = lift_images_host(planes, basis=basis, levels=lev).numpy()
            assert LC.same_bits(out[:, 0, 0].reshape(ll.shape), ll), (name, lev, "ll")
            assert LC.same_bits(out[:, 0, 1:].reshape(hi.shape), hi), (name, lev, "hi")
            only = lift_images_host(planes, basis=basis, levels=lev, ll_only=True).numpy()
            assert LC.same_bits(only.reshape(ll.shape), ll), (name, lev, "ll_only")


@pytest.mark.parametrize("basis", LC.BASES)
def test_twin_equals_the_oracle_on_float_input_over_the_small_sizes(basis):
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for H in LC.SMALL:
        for W in LC.SMALL:
            x = rng.standard_normal((1, 2, H, W)).astype(np.float32)
            x[0, 0, H // 2, W // 2] = -0.0
            layout = NHWC if (H + W) % 2 else NCHW
            src = LC.nhwc(x) if layout == NHWC else x
            for levels in (1, 2, 3):
                for ll_only in (0, 1):
                    rc, out = LC.run_cpu(lib, src, layout, 1, 2, H, W, None, None, basis, levels, ll_only)
                    assert rc == 0, lib.wv_last_error()
                    assert LC.same_bits(out, LC.expected(x, basis, levels, ll_only)), (H, W, levels, ll_only)


def all_bytes_image():
    """uint8 [1, 3, 18, 15]: every channel holds each of the 256 values, in a different order."""
    rng = np.random.default_rng(5)
    return np.stack([rng.permutation(np.arange(270) % 256).astype(np.uint8).reshape(18, 15) for _ in range(3)])[None]


@pytest.mark.parametrize("norm", [None, LC.IMAGENET, LC.UNEQUAL], ids=["plain", "imagenet", "unequal"])
def test_uint8_path_equals_torch_ops_then_oracle(norm):
    lib = _lib.load()
    x = all_bytes_image()
    assert all(len(np.unique(x[0, c])) == 256 for c in range(3))
    mean, std = norm if norm else (None, None)
    t = LC.to_tensor_normalize(x, mean, std).numpy()
    for layout in (NCHW, NHWC):
        src = LC.nhwc(x) if layout == NHWC else x
        rc, out = LC.run_cpu(lib, src, layout, 1, 3, 18, 15, mean, std, "haar", 0, 0)
        assert rc == 0 and LC.same_bits(out, t), layout                                  # levels = 0: the torch expression itself
        for basis in LC.BASES:
            for levels in (1, 2):
                for ll_only in (0, 1):
                    rc, out = LC.run_cpu(lib, src, layout, 1, 3, 18, 15, mean, std, basis, levels, ll_only)
                    assert rc == 0 and LC.same_bits(out, LC.expected(t, basis, levels, ll_only)), (layout, basis, levels, ll_only)
    # the pad comes after Normalize: a padded sample is +0.0, not normalize(0)
    if norm:
        rc, out = LC.run_cpu(lib, x[:, :, :3, :3], NCHW, 1, 3, 3, 3, mean, std, "haar", 1, 0)
        padded = np.pad(LC.to_tensor_normalize(x[:, :, :3, :3], mean, std).numpy(), [(0, 0), (0, 0), (0, 1), (0, 1)])
        assert rc == 0 and LC.same_bits(out, lifting_np.custom_transform(padded, 1, "haar"))


def test_argument_check_field_by_field():
    lib = _lib.load()
    EINVAL, ENOTSUP = -22, -95
    ok = dict(in_dtype=0, in_layout=1, B=2, C=3, H=8, W=8, basis=0, levels=1, ll_only=0)
    order = list(ok)

    def check(**kw):
        a = dict(ok, **kw)
        return lib.wv_lift_images_check(*[a[k] for k in order]), lib.wv_last_error().decode()

    assert check()[0] == 0 and check(B=0)[0] == 0 and check(levels=0)[0] == 0 and check(C=4, H=16384, W=16384, levels=16)[0] == 0
    for kw, code, text in (
            (dict(in_dtype=2), EINVAL, "in_dtype = 2"), (dict(in_layout=2), EINVAL, "in_layout = 2"), (dict(B=-1), EINVAL, "B = -1"),
            (dict(C=0), EINVAL, "C = 0"), (dict(H=0), EINVAL, "H = 0"), (dict(W=-3), EINVAL, "W = -3"), (dict(basis=2), EINVAL, "basis = 2"),
            (dict(levels=-1), EINVAL, "levels = -1"), (dict(ll_only=2), EINVAL, "ll_only = 2"),
            (dict(C=5), ENOTSUP, "C = 5 (limit 4)"), (dict(H=16385), ENOTSUP, "H = 16385 (limit 16384)"),
            (dict(W=16385), ENOTSUP, "W = 16385 (limit 16384)"), (dict(levels=17), ENOTSUP, "levels = 17 (limit 16)"),
            (dict(B=2 ** 30, C=4), ENOTSUP, "B * C")):
        rc, msg = check(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    # what the entry points add: to_tensor, mean / std
    x = np.zeros((1, 3, 4, 4), np.uint8)
    f = x.astype(np.float32)
    for src, to_tensor, mean, std, code, text in (
            (x, 2, None, None, EINVAL, "to_tensor = 2"), (x, 1, (0.5,) * 3, None, EINVAL, "mean and std"),
            (f, 1, None, None, EINVAL, "to_tensor = 1 scales 8-bit"), (x, 1, (0.5,) * 3, (1.0, 0.0, 1.0), EINVAL, "std[1] = 0"),
            (x, 1, (0.5, float("nan"), 0.5), (1.0,) * 3, EINVAL, "NaN"), (f, 0, (0.5,) * 3, (1.0,) * 3, ENOTSUP, "Normalize is folded")):
        rc, _ = LC.run_cpu(lib, src, NCHW, 1, 3, 4, 4, mean, std, "haar", 1, 0, to_tensor=to_tensor)
        assert rc == code and text in lib.wv_last_error().decode(), (to_tensor, mean, std, rc, lib.wv_last_error())
    assert lib.wv_lift_images_cpu(None, 0, 0, 1, 3, 4, 4, 1, None, None, 0, 1, 0, None) == EINVAL and b"NULL" in lib.wv_last_error()
    assert lib.wv_lift_images_cpu(None, 0, 0, 0, 3, 4, 4, 1, None, None, 0, 1, 0, None) == 0               # B = 0: nothing touched
    assert [lib.wv_lift_out_size(n, 0, 3) for n in (100, 75, 1)] == [13, 10, 1]
    assert [lib.wv_lift_out_size(n, 1, 2) for n in (50, 30, 1)] == [14, 8, 2] and lib.wv_lift_out_size(0, 0, 1) == 0
    assert lib.wv_lift_images_workspace_bytes(2, 3, 224, 224, 0, 1) == 0
    assert lib.wv_lift_images_workspace_bytes(2, 3, 224, 224, 0, 2) == 6 * 112 * 112 * 4
    assert lib.wv_lift_images_workspace_bytes(2, 3, 224, 224, 0, 3) == 6 * (112 * 112 + 56 * 56) * 4
    assert lib.wv_lift_images_tile(0) >= 2 and lib.wv_lift_images_tile(1) >= 2 and lib.wv_lift_images_tile(2) == 0


class _Images(torch.utils.data.Dataset):
    def __init__(self, images, transform):
        self.images, self.transform = images, transform

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.transform(self.images[i])


def per_image_expectation(img, size=256, crop=224, norm=LC.IMAGENET, basis="haar", levels=1):
    """Resize -> CenterCrop with PIL, ToTensor / Normalize as live torch ops, the lifting by the oracle."""
    from wvhash.transforms import CenterCrop, Resize
    arr = np.array(CenterCrop(crop)(Resize(size)(img)))
    t = LC.to_tensor_normalize(arr.transpose(2, 0, 1)[None], *norm).numpy()
    return LC.expected(t, basis, levels, 0)[0]


def test_custom_transform_runs_in_dataloader_workers_without_a_gpu():
    from wvhash.transforms import build_transform
    gpu_touched_before = torch.cuda.is_initialized()
    images = LC.pil_images(6)
    loader = torch.utils.data.DataLoader(_Images(images, build_transform(LC.CUB_DWT["test"])), batch_size=3, num_workers=2)
    got = torch.cat(list(loader))
    assert tuple(got.shape) == (6, 3, 4, 112, 112) and got.dtype == torch.float32
    for k, img in enumerate(images):
        assert LC.same_bits(got[k], per_image_expectation(img)), k
    if not torch.cuda.is_available():
        assert not torch.cuda.is_initialized()
    assert torch.cuda.is_initialized() == gpu_touched_before


def test_custom_transform_host_twin_with_device_cpu_and_its_refusal():
    from wvhash.transforms import CustomTransform
    x = torch.randn(3, 50, 30, generator=torch.Generator().manual_seed(5))
    for basis, levels in (("haar", 3), ("cdf97", 2)):
        for ll_only in (False, True):
            y = CustomTransform(decompose_levels=levels, basis=basis, ll_only=ll_only, device="cpu")(x)
            assert LC.same_bits(y, lifting_np.custom_transform(x.numpy(), levels, basis, ll_only=ll_only))
    y = CustomTransform(decompose_levels=1, basis="cdf97", coarse_only=False, device="cpu")(x[None])
    assert LC.same_bits(y, lifting_np.custom_transform(x.numpy()[None], 1, "cdf97", coarse_only=False))
    with pytest.raises(NotImplementedError):
        CustomTransform(decompose_levels=2, basis="haar", coarse_only=False, device="cpu")(x)


DEFER_NODES = [("cub_dwt-test", LC.CUB_DWT["test"], 224, (4, 3, 4, 112, 112)), ("cub_dwt-train", LC.CUB_DWT["train"], 224, (4, 3, 4, 112, 112)),
               ("cub_dwt_cdf97-test", LC.CUB_DWT_CDF97["test"], 448, (4, 3, 4, 224, 224)),
               ("cub_dwt_cdf97-train", LC.CUB_DWT_CDF97["train"], 448, (4, 3, 4, 224, 224)),
               ("basic-train", LC.BASIC["train"], 224, (4, 3, 224, 224)), ("basic-test", LC.BASIC["test"], 224, (4, 3, 224, 224))]


@pytest.mark.parametrize("name,node,side,shape", DEFER_NODES, ids=[n[0] for n in DEFER_NODES])
def test_deferred_tail_equals_the_per_image_pipeline(name, node, side, shape):
    from wvhash.transforms import (BaseWaveletTransform, RawItem, TensorTailTransform, build_transform, find_wavelet_transform,
                                   raw_collate)
    images = LC.pil_images(4, seed=21)
    torch.manual_seed(77)
    plain = build_transform(node, device="cpu")
    want = torch.stack([plain(img) for img in images])
    assert tuple(want.shape) == shape and want.dtype == torch.float32

    torch.manual_seed(77)
    deferred = build_transform(node, defer=True)
    plugin = find_wavelet_transform(deferred)
    assert isinstance(plugin, TensorTailTransform) and isinstance(plugin, BaseWaveletTransform) and plugin is deferred.transforms[-1]
    assert "ToTensor()" in repr(plugin) and ("Normalize(" in repr(plugin)) == ("Normalize" in node)
    assert ("CustomTransform(" in repr(plugin)) == ("CustomTransform" in node)
    items = [deferred(img) for img in images]
    assert all(it.dtype == torch.uint8 and tuple(it.shape) == (3, side, side) for it in items)
    assert LC.same_bits(plugin.apply_batch(torch.stack(items)), want)

    torch.manual_seed(77)
    on_device = build_transform(node, defer=True, sizing="device")
    raw = [on_device(img) for img in images]
    assert all(isinstance(it, RawItem) for it in raw)
    batch = raw_collate(raw)
    assert batch.out_shape == (4, side, side)
    assert LC.same_bits(find_wavelet_transform(on_device).apply_batch(batch), want)


def test_tensor_steps_ahead_of_geometry_cannot_be_deferred():
    from wvhash.transforms import CustomTransform, build_transform
    with pytest.raises(ValueError, match="'ToTensor'"):
        build_transform(LC.SDD_DWT_TRAIN, defer=True)
    with pytest.raises(ValueError, match="'ToTensor'"):
        build_transform(LC.SDD_DWT_TRAIN, defer=True, sizing="device")
    steps = build_transform(LC.SDD_DWT_TRAIN).transforms                      # defer=False: the node builds, step by step
    assert [type(s).__name__ for s in steps] == list(LC.SDD_DWT_TRAIN) and isinstance(steps[1], CustomTransform)
    with pytest.raises(NotImplementedError):
        build_transform({"ToTensor": {}, "CustomTransform": {"decompose_levels": 2, "coarse_only": False}}, defer=True)
    with pytest.raises(ValueError, match="division by zero"):
        build_transform({"ToTensor": {}, "Normalize": {"mean": [0.5], "std": [0.0]}}, defer=True)


def test_local_to_tensor_and_normalize():
    from wvhash.transforms import Normalize, ToTensor
    arr = np.random.default_rng(2).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    t = ToTensor()(Image.fromarray(arr))
    assert t.dtype == torch.float32 and LC.same_bits(t, torch.from_numpy(arr).permute(2, 0, 1).float().div(255))
    assert tuple(ToTensor()(Image.fromarray(arr[:, :, 0])).shape) == (1, 5, 7)
    n = Normalize(*LC.IMAGENET)(t)
    assert LC.same_bits(n, LC.to_tensor_normalize(arr.transpose(2, 0, 1), *LC.IMAGENET)) and n.data_ptr() != t.data_ptr()
    assert Normalize(*LC.IMAGENET, inplace=True)(t).data_ptr() == t.data_ptr()
    with pytest.raises(ValueError, match="std evaluated to zero"):
        Normalize([0.5] * 3, [1.0, 0.0, 1.0])(t.clone())
    with pytest.raises(TypeError):
        Normalize([0.5] * 3, [1.0] * 3)(torch.zeros(3, 4, 4, dtype=torch.uint8))


def test_random_crop_draw_order_and_refusals():
    from wvhash.transforms import LazyImage, RandomCrop
    img = Image.fromarray(np.random.default_rng(4).integers(0, 256, (40, 60, 3), dtype=np.uint8))
    torch.manual_seed(9)
    got = RandomCrop(size=(24, 32))(img)
    torch.manual_seed(9)
    i = torch.randint(0, 40 - 24 + 1, size=(1,)).item()             # the row first, then the column
    j = torch.randint(0, 60 - 32 + 1, size=(1,)).item()
    assert got.size == (32, 24) and np.array_equal(np.array(got), np.array(img)[i:i + 24, j:j + 32])
    torch.manual_seed(9)
    state = torch.get_rng_state()
    same = RandomCrop(size=(40, 60))(img)                           # equal sizes: no draw
    assert torch.equal(torch.get_rng_state(), state) and np.array_equal(np.array(same), np.array(img))
    assert RandomCrop(24).size == (24, 24) and RandomCrop([24]).size == (24, 24)
    torch.manual_seed(9)
    lazy = RandomCrop(size=(24, 32))(LazyImage(img))                # recorded, not cropped
    assert lazy.size == (32, 24) and lazy.ops == [("crop", (j, i, 32, 24))]
    with pytest.raises(ValueError, match="larger than input image size"):
        RandomCrop(64)(img)
    for kw in (dict(padding=4), dict(pad_if_needed=True)):
        with pytest.raises(ValueError):
            RandomCrop(24, **kw)
