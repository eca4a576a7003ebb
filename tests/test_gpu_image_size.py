"""Image sizing on the GPU: the kernel against its host twin byte for byte on one ragged batch that takes every branch in
one launch (tests/test_host_image_size.py holds the twin to Pillow on the same cases), then the path above it: size_images
-> swt2d against swt2d of the PIL-sized batch, evaluate() and a training step on sizing="device" against sizing="host"."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import image_size_cases as C
from wvhash import _lib, synth
from wvhash.transforms import build_transform, sizing, size_images, size_images_host, swt2d

pytestmark = pytest.mark.gpu
DT = sizing.STAGE_DTYPE

TEST_NODE = {"Resize": {"size": 256}, "CenterCrop": {"size": 224}}
TRAIN_NODE = {"Resize": {"size": 256}, "RandomResizedCrop": {"size": 224}, "RandomHorizontalFlip": {"p": 0.5}}
SIZES = ((500, 375), (375, 500), (200, 180))


def node(geometry, level=1, wavelet="haar"):
    return dict(geometry, SWTTransform={"level": level, "wavelet": wavelet})


def test_kernel_equals_host_twin_on_one_ragged_batch():
    lib = _lib.require_gpu()
    cases = C.ragged_cases()
    src, rec, dst_bytes, outs = C.pack(cases, DT, src_gap=1, dst_gap=5)             # odd offsets; gaps must stay untouched
    ref = np.full(dst_bytes, 0xAB, np.uint8)
    assert lib.wv_image_size_cpu(ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(ref.ctypes.data),
                                 ctypes.c_void_p(rec.ctypes.data), len(rec)) == 0, lib.wv_last_error()
    assert lib.wv_image_size_check(ctypes.c_void_p(rec.ctypes.data), len(rec)) == 0
    d_src = torch.from_numpy(src).cuda()
    d_rec = torch.from_numpy(rec.view(np.int32).reshape(len(rec), -1).copy()).cuda()
    d_dst = torch.full((dst_bytes,), 0xAB, dtype=torch.uint8, device="cuda")
    max_k = C.max_ksize(rec)
    assert max_k == 257                                                               # the 64 -> 1 rows bicubic image
    rc = lib.wv_image_size(_lib.ptr(d_src), _lib.ptr(d_dst), _lib.ptr(d_rec), len(rec), int(rec["out_h"].max()),
                           int(rec["out_w"].max()), max_k, _lib.stream_ptr())
    assert rc == 0, lib.wv_last_error()
    got = d_dst.cpu().numpy()
    for i, (g, r) in enumerate(zip(C.unpack(got, outs), C.unpack(ref, outs))):
        assert np.array_equal(g, r), (i, cases[i][1], int(np.abs(g.astype(int) - r).max()))
    assert np.array_equal(got, ref)                                                   # ... and the gaps between the images
    # the same batch without the heavy down-scales: large tiles, several row tiles per image (500 x 375 -> 224 x 224 window)
    keep = [i for i in range(len(rec)) if C.max_ksize(rec[i:i + 1]) <= 11]
    assert 24 in keep and len(keep) >= 20                                             # the twelve pairs: 0..23, then the variants
    sub = np.ascontiguousarray(rec[keep])
    d_dst.fill_(0xAB)
    rc = lib.wv_image_size(_lib.ptr(d_src), _lib.ptr(d_dst), _lib.ptr(torch.from_numpy(sub.view(np.int32).reshape(len(sub), -1).copy()).cuda()),
                           len(sub), int(sub["out_h"].max()), int(sub["out_w"].max()), C.max_ksize(sub), _lib.stream_ptr())
    assert rc == 0, lib.wv_last_error()
    got = d_dst.cpu().numpy()
    for i in keep:
        off, h, w = outs[i]
        assert np.array_equal(got[off:off + 3 * h * w], ref[off:off + 3 * h * w]), (i, cases[i][1])


def pil_images(n, seed0=0):
    return [Image.fromarray(C.image(*SIZES[i % 3], "noise", seed0 + i)) for i in range(n)]


@pytest.mark.parametrize("wavelet,level", [("haar", 1), ("db2", 3)])
def test_sized_batch_through_swt_equals_pil_sized_batch(wavelet, level):
    imgs = pil_images(5)
    cfg = node(TEST_NODE, level, wavelet)
    host = torch.stack([build_transform(cfg, defer=True)(im) for im in imgs])        # uint8 [5, 3, 224, 224], PIL
    tf = build_transform(cfg, defer=True, sizing="device")
    rb = sizing.raw_collate([tf(im) for im in imgs]).pin_memory().cuda(non_blocking=True)
    sized = size_images(rb)
    assert sized.is_cuda and tuple(sized.shape) == (5, 224, 224, 3)
    assert torch.equal(sized.cpu(), host.permute(0, 2, 3, 1))
    assert torch.equal(sized.cpu(), size_images_host(sizing.raw_collate([tf(im) for im in imgs])))
    a = swt2d(sized, wavelet, level, channels_last=True)
    b = swt2d(host.cuda(), wavelet, level)
    assert torch.equal(a, b)
    assert torch.equal(tf.transforms[-1].apply_batch(rb), b)                           # the plugin takes the RawBatch itself


def test_train_node_two_stage_batch_equals_pil():
    imgs = pil_images(6, seed0=20)
    cfg = node(TRAIN_NODE)
    torch.manual_seed(7)
    host = torch.stack([build_transform(cfg, defer=True)(im) for im in imgs])
    torch.manual_seed(7)
    tf = build_transform(cfg, defer=True, sizing="device")
    rb = sizing.raw_collate([tf(im) for im in imgs])
    assert len(rb.launches) == 2                                                      # Resize, then crop + resize + flip
    assert torch.equal(size_images(rb.cuda()).cpu(), host.permute(0, 2, 3, 1))


@pytest.fixture(scope="module")
def net():
    from wvhash.models import SharedDinoHashing
    from wvhash.models.vit import tiny_vit
    torch.manual_seed(0)
    fusion = {"type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "num_queries": 4,
              "sub_band_dropout_p": 0, "ortho_weight": 0.1}
    m = SharedDinoHashing({"name": "dinov2_vits14", "frozen": True}, fusion, {"nbits": 64}, backbone=tiny_vit())
    m.hash_fc.weight.data.mul_(50)
    for name, prm in m.named_parameters():
        if name.endswith(".gamma"):
            prm.data.fill_(1.0)
    return m.cuda().eval()


def test_evaluate_gives_identical_codes_and_metrics_with_both_sizings(net, tmp_path):
    """Mixed-size image FILES through MIRFlickrHashing and the YAML pipeline, as tests/test_gpu_evaluate.py writes them."""
    from wvhash.datasets import MIRFlickrHashing
    from wvhash.engine import evaluate
    from wvhash.engine.evaluate import get_tester
    (tmp_path / "images").mkdir()
    for fname, n, seed in (("test.txt", 4, 3), ("database.txt", 8, 4)):
        labels = synth.multi_hot_labels(n, 38, 0.25, seed)
        with open(tmp_path / fname, "w") as f:
            for i in range(n):
                name = f"{fname[:2]}{i}.png"
                Image.fromarray(C.image(*SIZES[i % 3], "noise", 10 * seed + i)).save(tmp_path / "images" / name)
                f.write(name + " " + " ".join(str(int(v)) for v in labels[i]) + "\n")
    results, codes = {}, {}
    for how in ("host", "device"):
        tf = build_transform(node(TEST_NODE), defer=True, sizing=how)
        dts = {"test": MIRFlickrHashing(str(tmp_path), "test", tf), "gallery": MIRFlickrHashing(str(tmp_path), "gallery", tf)}
        results[how] = evaluate(net, test_dataset=dts, epoch=0, batch_size=5, num_workers=0, k=6, distance_metric="hamming",
                                pr_rc_path=None, exclude=["mean_reciprocal_rank", "precision_at_1", "r_precision"])
        tester = get_tester(batch_size=5, num_workers=0, k=6, distance_metric="hamming")
        codes[how] = [tester.get_all_embeddings(dts[s], net)[0].cpu() for s in ("test", "gallery")]
    assert set(codes["host"][1].unique().tolist()) <= {-1.0, 1.0} and codes["host"][1].unique(dim=0).shape[0] > 1
    for a, b in zip(codes["host"], codes["device"]):
        assert torch.equal(a, b)
    assert results["host"] == results["device"] and "maphashing_level0" in results["host"]["test"]


def test_training_step_takes_the_raw_batch():
    from wvhash.engine import backward_step
    from wvhash.losses import HashLoss
    from wvhash.models import SharedDinoHashing
    from wvhash.models.vit import tiny_vit
    imgs = pil_images(4, seed0=40)
    y = synth.multi_hot_labels(4, 38, 0.10, 1)
    logs = {}
    for how in ("host", "device"):
        torch.manual_seed(0)
        fusion = {"type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "num_queries": 4, "dropout": 0.0,
                  "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
        m = SharedDinoHashing({"name": "dinov2_vits14", "frozen": True}, fusion, {"nbits": 64}, backbone=tiny_vit())
        tf = build_transform(node(TRAIN_NODE), defer=True, sizing=how)
        m = m.cuda().train().bind_transform(tf)
        crit = HashLoss(num_classes=38, embedding_size=64).cuda()
        torch.manual_seed(11)
        items = [tf(im) for im in imgs]
        x = torch.stack(items) if how == "host" else sizing.raw_collate(items)
        torch.manual_seed(12)
        logs[how] = backward_step(m, x, y, [(crit, 1.0)], autocast_dtype=None)
        grad = m.hash_fc.weight.grad.clone()
        logs[how]["grad"] = grad
    assert torch.equal(logs["host"].pop("grad"), logs["device"].pop("grad"))
    assert logs["host"] == logs["device"] and "total_loss" in logs["host"]
