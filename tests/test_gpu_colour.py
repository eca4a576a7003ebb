"""Colour jitter on the GPU: the kernel against its host twin byte for byte (tests/test_host_colour.py holds the twin to
Pillow on the same cases) on one ragged buffer that takes every branch in one call, on every colour, and on a sum above 32
bits; then the path above it: size_images of the VOC train node -> swt2d against the PIL pipeline, and a training step on
sizing="device" against sizing="host"."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import colour_cases as C
from wvhash import _lib, synth
from wvhash.transforms import build_transform, sizing, size_images, size_images_host, swt2d

pytestmark = pytest.mark.gpu
DT = sizing.COLOUR_DTYPE


def device_records(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), -1).copy()).cuda()


def launch(lib, d_buf, rec, d_rec=None):
    d_rec = device_records(rec) if d_rec is None else d_rec
    nbytes = lib.wv_colour_jitter_workspace_bytes(len(rec))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.wv_colour_jitter(_lib.ptr(d_buf), _lib.ptr(d_rec), len(rec), int(rec["h"].max()), int(rec["w"].max()), _lib.ptr(ws),
                              ctypes.c_size_t(nbytes), _lib.stream_ptr())
    assert rc == 0, lib.wv_last_error()
    return d_buf


def twin(lib, buf, rec):
    ref = buf.copy()
    assert lib.wv_colour_jitter_cpu(ctypes.c_void_p(ref.ctypes.data), ctypes.c_void_p(rec.ctypes.data), len(rec)) == 0, lib.wv_last_error()
    return ref


def test_kernel_equals_host_twin_on_one_ragged_buffer():
    lib = _lib.require_gpu()
    cases = C.ragged_cases()
    buf, rec = C.pack(cases, DT)                                                      # 0xAB between the images and behind the rows
    assert lib.wv_colour_jitter_check(ctypes.c_void_p(rec.ctypes.data), len(rec)) == 0, lib.wv_last_error()
    # what the one call must cover: every width, an image of several tiles (1024 groups of four pixels each), images without
    # contrast (no statistics work), an empty chain, every offset residue, padded rows
    assert {int(w) for w in rec["w"]} == set(C.WIDTHS)
    assert ((rec["h"] * ((rec["w"] + 3) // 4)) > 3 * 1024).any()
    assert any(n and C.CONTRAST not in k[:n] for n, k in zip(rec["n_ops"], rec["kind"].tolist()))
    assert (rec["n_ops"] == 0).any() and {int(o) % 4 for o in rec["offset"]} == {0, 1, 2, 3}
    assert (rec["row_bytes"] > 3 * rec["w"]).any()
    ref = twin(lib, buf, rec)
    got = launch(lib, torch.from_numpy(buf).cuda(), rec).cpu().numpy()
    for i, (g, r) in enumerate(zip(C.unpack(got, rec), C.unpack(ref, rec))):
        assert np.array_equal(g, r), (i, cases[i][0].shape, cases[i][1], int(np.abs(g.astype(int) - r).max()))
    assert np.array_equal(got, ref)                                                   # ... and the bytes that belong to no image
    again = launch(lib, torch.from_numpy(buf).cuda(), rec)                            # the same launch twice: the same bytes
    assert torch.equal(again, torch.from_numpy(got).cuda())


def test_saturation_of_every_colour_equals_host_twin():
    lib = _lib.require_gpu()
    f = C.seeded_factor(11)
    buf, rec = C.pack([(C.all_colours(), [(C.SATURATION, f)])], DT)
    got = launch(lib, torch.from_numpy(buf).cuda(), rec).cpu().numpy()
    assert np.array_equal(got, twin(lib, buf, rec))


def test_contrast_sum_above_32_bits_equals_host_twin():
    lib = _lib.require_gpu()
    buf, rec = C.pack([(np.full((4200, 4200, 3), 255, np.uint8), [(C.CONTRAST, 0.75)])], DT)
    got = launch(lib, torch.from_numpy(buf).cuda(), rec).cpu().numpy()
    assert np.array_equal(got, twin(lib, buf, rec)) and int(got.min()) == 255        # a 32-bit sum gives a mean of 11


def test_entry_point_checks_its_own_arguments():
    lib = _lib.require_gpu()
    one = ctypes.c_void_p(16)                                                         # never dereferenced
    assert lib.wv_colour_jitter(one, one, 0, 0, 0, None, 0, None) == 0
    for args, code, words in (((one, one, -1, 4, 4, one, 64, None), -22, "n = -1"),
                              ((None, one, 2, 4, 4, one, 64, None), -22, "NULL"),
                              ((one, one, 2, 0, 4, one, 64, None), -22, "max_h = 0"),
                              ((one, one, 2, 4, 16385, one, 64, None), -95, "max_w = 16385"),
                              ((one, one, 2, 4, 4, None, 64, None), -22, "workspace"),
                              ((one, one, 2, 4, 4, one, 8, None), -12, "need 16")):
        assert lib.wv_colour_jitter(*args) == code and words in lib.wv_last_error().decode(), (args, lib.wv_last_error())


def pil_images(n, seed0=0):
    return [Image.fromarray(C.image(*C.SIZES[i % 3], seed0 + i)) for i in range(n)]


@pytest.fixture(scope="module")
def voc_batch():
    """Five images through the VOC train node with one seed: the PIL batch and the RawBatch (haar, level 1: fix_size adds
    nothing at 224 for any level the tests use)."""
    imgs = pil_images(5)
    cfg = C.voc_node()
    torch.manual_seed(7)
    th = build_transform(cfg, defer=True)
    host = torch.stack([th(im) for im in imgs])                                       # uint8 [5, 3, 224, 224], PIL
    torch.manual_seed(7)
    tf = build_transform(cfg, defer=True, sizing="device")
    rb = sizing.raw_collate([tf(im) for im in imgs])
    return host, rb


def test_voc_node_sized_on_the_gpu_equals_twin_and_pil(voc_batch):
    host, rb = voc_batch
    assert rb.colour_launches == ((0, 0, 0, 0), (0, 5, 224, 224))
    d = rb.pin_memory().cuda(non_blocking=True)
    assert d.colour.is_cuda and d.colour_launches == rb.colour_launches
    sized = size_images(d)
    assert sized.is_cuda and tuple(sized.shape) == (5, 224, 224, 3)
    assert torch.equal(sized.cpu(), size_images_host(rb))
    assert torch.equal(sized.cpu(), host.permute(0, 2, 3, 1))
    assert torch.equal(size_images(d), sized)


@pytest.mark.parametrize("wavelet,level", [("haar", 1), ("db2", 3)])
def test_voc_node_through_swt_equals_pil_batch(voc_batch, wavelet, level):
    host, rb = voc_batch
    d = rb.cuda()
    b = swt2d(host.cuda(), wavelet, level)
    assert torch.equal(swt2d(size_images(d), wavelet, level, channels_last=True), b)
    plugin = build_transform(C.voc_node(level, wavelet), defer=True, sizing="device").transforms[-1]
    assert torch.equal(plugin.apply_batch(d), b)                                      # the plugin takes the RawBatch itself


def test_training_step_takes_the_voc_raw_batch():
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
        tf = build_transform(C.voc_node(), defer=True, sizing=how)
        m = m.cuda().train().bind_transform(tf)
        crit = HashLoss(num_classes=38, embedding_size=64).cuda()
        torch.manual_seed(11)
        items = [tf(im) for im in imgs]
        x = torch.stack(items) if how == "host" else sizing.raw_collate(items)
        if how == "device":
            assert x.colour is not None and x.colour_launches[1][1] == 4
        torch.manual_seed(12)
        logs[how] = backward_step(m, x, y, [(crit, 1.0)], autocast_dtype=None)
        logs[how]["grad"] = m.hash_fc.weight.grad.clone()
        with torch.no_grad():
            logs[how]["codes"] = m.eval()(x.cuda()).cpu()                              # eval mode: the sign codes
    assert torch.equal(logs["host"].pop("grad"), logs["device"].pop("grad"))
    codes = logs["host"].pop("codes")
    assert set(codes.unique().tolist()) <= {-1.0, 1.0} and torch.equal(codes, logs["device"].pop("codes"))
    assert logs["host"] == logs["device"] and "total_loss" in logs["host"]
