"""Image sizing on the host (no GPU): wv_image_size_cpu against the live Pillow, bit for bit; the recorder of
build_transform(..., sizing="device") against the PIL pipeline of sizing="host"; the argument check field by field; the
host twin over a ragged batch under AddressSanitizer + UBSan in a stand-alone program.  Every comparison is exact uint8
equality."""
import ctypes
import os
import subprocess

import numpy as np
import PIL
import pytest
import torch
from PIL import Image, ImageOps

import image_size_cases as C
from wvhash import _lib
from wvhash.transforms import build_transform, pil_ops, sizing, size_images_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = sizing.STAGE_DTYPE

TEST_NODE = {"Resize": {"size": 256}, "CenterCrop": {"size": 224}, "SWTTransform": {"level": 1, "wavelet": "haar"}}
TRAIN_NODE = {"Resize": {"size": 256}, "RandomResizedCrop": {"size": 224}, "RandomHorizontalFlip": {"p": 0.5},
              "SWTTransform": {"level": 1, "wavelet": "haar"}}                       # config/transform/basic_swt.yaml
CIFAR_NODE = {"Resize": {"size": [224, 224]}, "SWTTransform": {"level": 1, "wavelet": "haar"}}   # cifar_swt.yaml: test
LEVEL3_NODE = {"SWTTransform": {"level": 3, "wavelet": "db2"}}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def one(lib, arr, **kw):
    st = C.stage(arr, **kw)
    return C.run_cpu(lib, [(arr, st)], DT)[0], st


@pytest.mark.parametrize("kind", ["noise", "binary"])
@pytest.mark.parametrize("filt", [C.BILINEAR, C.BICUBIC])
def test_resize_equals_pillow(lib, filt, kind):
    pairs = C.FIXED_PAIRS + C.random_pairs()
    assert len(pairs) == 12 + 150
    for i, (w, h, ow, oh) in enumerate(pairs):
        arr = C.image(w, h, kind, i)
        got, _ = one(lib, arr, out_wh=(ow, oh), filt=filt)
        ref = np.array(Image.fromarray(arr).resize((ow, oh), C.FILTERS[filt]))
        assert np.array_equal(got, ref), (w, h, ow, oh, filt, kind)


@pytest.mark.parametrize("filt", [C.BILINEAR, C.BICUBIC])
def test_crop_window_pad_and_flip_equal_pillow(lib, filt):
    arr = C.image(61, 45, "noise", 5)
    img = Image.fromarray(arr)
    # crop with a non-zero origin is a new image: bounds clamp at the crop's edge
    got, _ = one(lib, arr, out_wh=(20, 17), filt=filt, crop=(7, 5, 40, 33))
    assert np.array_equal(got, np.array(img.crop((7, 5, 47, 38)).resize((20, 17), C.FILTERS[filt])))
    got, _ = one(lib, arr, out_wh=(25, 31), filt=filt, crop=(21, 12, 40, 33))        # touching the last row and column
    assert np.array_equal(got, np.array(img.crop((21, 12, 61, 45)).resize((25, 31), C.FILTERS[filt])))
    # window = .resize(...).crop(...)
    got, _ = one(lib, arr, out_wh=(30, 22), filt=filt, window=(3, 4, 21, 15))
    assert np.array_equal(got, np.array(img.resize((30, 22), C.FILTERS[filt]).crop((3, 4, 24, 19))))
    # a window overhanging a too small image = pil_ops.CenterCrop (zero pad)
    for size in ((40, 40), (18, 50), (60, 12)):                                      # (h, w): pad both, pad width, pad height
        small = img.resize((30, 22), C.FILTERS[filt])
        ref = np.array(pil_ops.CenterCrop(size)(small))
        lazy = pil_ops.CenterCrop(size)(sizing.LazyImage(img).resize((30, 22), C.FILTERS[filt]))
        (op, (x, y, w, h)), = lazy.ops[1:]
        got, _ = one(lib, arr, out_wh=(30, 22), filt=filt, window=(x, y, w, h))
        assert got.shape == ref.shape == size + (3,) and np.array_equal(got, ref), size
    # flip = ImageOps.mirror, of the written window
    got, _ = one(lib, arr, out_wh=(30, 22), filt=filt, window=(-2, 5, 20, 30), flip=1)
    assert np.array_equal(got, np.array(ImageOps.mirror(img.resize((30, 22), C.FILTERS[filt]).crop((-2, 5, 18, 35)))))
    # nothing resampled: copy, crop and mirror only
    got, _ = one(lib, arr, window=(10, 3, 30, 40), flip=1)
    assert np.array_equal(got, np.array(ImageOps.mirror(img.crop((10, 3, 40, 43)))))


def test_ragged_batch_equals_pillow_case_by_case(lib):
    cases = C.ragged_cases()
    outs = C.run_cpu(lib, cases, DT)
    for i, ((arr, st), got) in enumerate(zip(cases, outs)):
        assert np.array_equal(got, C.pillow_stage(arr, st)), (i, st)


def test_golden_pins_the_pillow_version_that_wrote_it(lib, golden_dir):
    g = np.load(os.path.join(golden_dir, "image_size_golden.npz"))
    for i in range(int(g["n"])):
        arr, v = g[f"in_{i}"], [int(x) for x in g[f"stage_{i}"]]
        st = {"crop": tuple(v[0:4]), "res": tuple(v[4:6]), "win": tuple(v[6:10]), "filter": v[10], "flip": v[11]}
        live, stored = C.pillow_stage(arr, st), g[f"out_{i}"]
        assert np.array_equal(live, stored), (
            f"Pillow changed: Pillow {PIL.__version__} no longer reproduces case {i} as Pillow {g['pillow_version']} "
            "resampled it; the library reproduces the stored version's arithmetic")
        assert np.array_equal(C.run_cpu(lib, [(arr, st)], DT)[0], stored), i


def pil_image(w, h, seed):
    return Image.fromarray(C.image(w, h, "noise", seed))


def host_and_device(node, img):
    host = build_transform(node, defer=True)(img)                                    # uint8 [3, H, W], PIL sizing
    item = build_transform(node, defer=True, sizing="device")(img)
    dev = size_images_host(sizing.raw_collate([item]))
    return host.permute(1, 2, 0), dev[0], item


@pytest.mark.parametrize("w,h", [(500, 375), (375, 500), (200, 180), (224, 224), (256, 300)])
def test_recorded_pipelines_equal_the_pil_pipelines(w, h):
    img = pil_image(w, h, 7)
    for node in (TEST_NODE, CIFAR_NODE):
        host, dev, item = host_and_device(node, img)
        assert tuple(dev.shape) == (224, 224, 3) and torch.equal(host, dev), node
        # one stage, whatever the steps; none when every step returns the image unchanged (Resize [224, 224] of 224 x 224)
        assert len(item.stages) == (0 if node is CIFAR_NODE and (w, h) == (224, 224) else 1)
        if node is TEST_NODE and w == 256:                                           # Resize(256) is a no-op: a window only
            assert int(item.stages[0]["res_w"]) == int(item.stages[0]["crop_w"]) == 256
        assert tuple(item.pixels.shape) == (h, w, 3)                                 # the worker did not touch the pixels
    small = pil_image(180, 150, 8)                                                   # Resize(200) -> 240 x 200: padded window
    node = {"Resize": {"size": 200}, "CenterCrop": {"size": 224}, "SWTTransform": {"level": 1, "wavelet": "haar"}}
    host, dev, item = host_and_device(node, small)
    assert torch.equal(host, dev) and len(item.stages) == 1 and int(item.stages[0]["win_y"]) < 0


def test_fix_size_is_recorded_as_a_bicubic_stage():
    img = pil_image(225, 30, 9)
    host, dev, item = host_and_device(LEVEL3_NODE, img)
    assert tuple(dev.shape) == (32, 232, 3) and torch.equal(host, dev)
    assert len(item.stages) == 1 and int(item.stages[0]["filter"]) == C.BICUBIC
    # after a padded window fix_size cannot join the stage: two stages, the second reads the first's output
    node = {"CenterCrop": {"size": [40, 230]}, "SWTTransform": {"level": 3, "wavelet": "db2"}}
    host, dev, item = host_and_device(node, img)
    assert tuple(dev.shape) == (40, 232, 3) and torch.equal(host, dev) and len(item.stages) == 2


def test_random_call_sequences_equal_their_replay_on_pil():
    rng = np.random.default_rng(3)
    for trial in range(150):
        img = pil_image(int(rng.integers(20, 90)), int(rng.integers(20, 90)), trial)
        lazy = sizing.LazyImage(img)
        for _ in range(int(rng.integers(1, 6))):
            w, h = lazy.size
            kind = rng.integers(0, 3)
            if kind == 0:
                lazy = lazy.resize((int(rng.integers(max(1, w // 3), 2 * w)), int(rng.integers(max(1, h // 3), 2 * h))),
                                   Image.BILINEAR if rng.integers(0, 2) else Image.BICUBIC)
            elif kind == 1:
                x, y = int(rng.integers(-4, w)), int(rng.integers(-4, h))
                lazy = lazy.crop((x, y, x + int(rng.integers(1, w + 5)), y + int(rng.integers(1, h + 5))))
            else:
                lazy = lazy.transpose(Image.FLIP_LEFT_RIGHT)
        got = size_images_host(sizing.raw_collate([lazy.to_item()]))[0].numpy()
        assert np.array_equal(got, np.array(lazy.materialize())), (trial, lazy.ops)


def test_train_node_builds_and_both_sizings_draw_and_size_alike():
    tf_host = build_transform(TRAIN_NODE, defer=True)
    tf_dev = build_transform(TRAIN_NODE, defer=True, sizing="device")
    assert tuple(build_transform(TRAIN_NODE, device="cpu")(pil_image(500, 375, 1)).shape) == (3, 4, 224, 224)
    imgs = [pil_image(*((500, 375), (375, 500), (300, 260), (640, 200))[i % 4], seed=i) for i in range(20)]
    torch.manual_seed(1234)
    host = [tf_host(im) for im in imgs]
    state_host = torch.get_rng_state()
    torch.manual_seed(1234)
    items = [tf_dev(im) for im in imgs]
    assert torch.equal(state_host, torch.get_rng_state())                           # the RNG was consumed identically
    dev = size_images_host(sizing.raw_collate(items))                                # one ragged batch of 20
    assert tuple(dev.shape) == (20, 224, 224, 3)
    flips = 0
    for i in range(20):
        assert torch.equal(host[i].permute(1, 2, 0), dev[i]), i
        assert len(items[i].stages) == 2                                             # Resize, then crop + resize (+ flip)
        flips += int(items[i].stages[-1]["flip"])
    assert 0 < flips < 20


def test_images_outside_the_kernel_are_sized_in_the_worker():
    img = pil_image(3000, 40, 2)                                                     # 3000 -> 40 columns: a 75x down-scale
    node = {"Resize": {"size": [40, 40]}, "SWTTransform": {"level": 1, "wavelet": "haar"}}
    host, dev, item = host_and_device(node, img)
    assert len(item.stages) == 0 and tuple(item.pixels.shape) == (40, 40, 3) and torch.equal(host, dev)
    both = sizing.raw_collate([item, build_transform(node, defer=True, sizing="device")(pil_image(90, 70, 3))])
    assert torch.equal(size_images_host(both)[0], dev)                               # sized and unsized images share a batch
    with pytest.raises(ValueError, match="defer=True"):
        build_transform(TEST_NODE, sizing="device")


def test_raw_batch_collates_dict_items_and_moves_as_one():
    tf = build_transform(TEST_NODE, defer=True, sizing="device")
    items = [{"image": tf(pil_image(300 + 10 * i, 260, i)), "label": torch.tensor([i, 1]), "path": str(i)} for i in range(3)]
    batch = sizing.raw_collate(items)
    rb = batch["image"]
    assert isinstance(rb, sizing.RawBatch) and len(rb) == 3 and batch["label"].shape == (3, 2) and batch["path"] == ["0", "1", "2"]
    assert rb.desc.dtype == torch.int32 and rb.desc.shape == (3, 20) and rb.data.dtype == torch.uint8 and not rb.is_cuda
    moved = rb.to("cpu")
    assert torch.equal(size_images_host(moved), size_images_host(rb)) and moved.launches == rb.launches


def test_packed_batches_equal_the_stored_ones_byte_for_byte(golden_dir):
    """raw_collate packs what it packed when tests/golden/raw_batch_golden.npz was written: every array and every tuple of
    a VOC train batch (two stage indices, a colour table), an eval batch (no colour table) and a batch that mixes a recorded
    image with one sized by PIL in the worker (identity record)."""
    import colour_cases
    g = np.load(os.path.join(golden_dir, "raw_batch_golden.npz"))
    batches = colour_cases.raw_batches()
    got = colour_cases.raw_batch_arrays(batches)
    assert sorted(got) == sorted(g.files)
    for key in g.files:
        assert got[key].dtype == g[key].dtype and got[key].shape == g[key].shape and np.array_equal(got[key], g[key]), key
    assert "voc_data_sha256" in g.files and "mixed_data" in g.files and bool(g["voc_has_colour"]) and not bool(g["eval_has_colour"])
    assert len(batches["mixed"].launches) == 1 and batches["mixed"].colour_launches == ((0, 1, 30, 40),)


class _Items(torch.utils.data.Dataset):
    def __init__(self, tf):
        self.tf = tf

    def __len__(self):
        return 5

    def __getitem__(self, i):
        return {"image": self.tf(pil_image(260 + 20 * i, 300, i)), "label": torch.tensor([float(i)]), "path": str(i)}


def test_raw_batches_come_out_of_dataloader_workers():
    """The workers record, collate in the worker, and the RawBatch crosses the process boundary as tensors."""
    ds = _Items(build_transform(TEST_NODE, defer=True, sizing="device"))
    ref = torch.stack([build_transform(TEST_NODE, defer=True)(pil_image(260 + 20 * i, 300, i)) for i in range(5)])
    dl = torch.utils.data.DataLoader(ds, batch_size=3, num_workers=1, collate_fn=sizing.raw_collate)
    got = torch.cat([size_images_host(b["image"]) for b in dl])
    assert torch.equal(got, ref.permute(0, 2, 3, 1))


def base_record():
    rec = np.zeros(1, dtype=DT)
    r = rec[0]
    r["src_h"], r["src_w"], r["src_row_bytes"] = 40, 50, 150
    r["crop_y"], r["crop_x"], r["crop_h"], r["crop_w"] = 2, 3, 30, 40
    r["res_h"], r["res_w"] = 20, 25
    r["win_y"], r["win_x"], r["out_h"], r["out_w"] = -1, 2, 24, 20
    r["dst_row_bytes"], r["filter"], r["flip"] = 60, C.BILINEAR, 0
    return rec


REJECTED = [(f, 0, -22) for f in ("src_h", "src_w", "crop_h", "crop_w", "res_h", "res_w", "out_h", "out_w")] + [
    ("src_h", 16385, -95), ("src_w", 16385, -95), ("res_h", 16385, -95), ("res_w", 16385, -95), ("out_h", 16385, -95),
    ("out_w", 16385, -95), ("crop_y", -1, -22), ("crop_y", 11, -22), ("crop_x", -1, -22), ("crop_x", 11, -22),
    ("filter", 1, -22), ("filter", 0, -22), ("flip", 2, -22), ("src_row_bytes", 149, -22), ("dst_row_bytes", 59, -22),
    ("src_offset", -1, -22), ("dst_offset", -8, -22), ("win_y", 16385, -95), ("win_x", -16385, -95)]


@pytest.mark.parametrize("field,value,code", REJECTED)
def test_check_rejects_every_field_by_name(lib, field, value, code):
    rec = base_record()
    assert lib.wv_image_size_check(ctypes.c_void_p(rec.ctypes.data), 1) == 0
    rec[0][field] = value
    if field in ("src_w", "out_w") and value > 16384:
        rec[0]["src_row_bytes" if field == "src_w" else "dst_row_bytes"] = 3 * value
    assert lib.wv_image_size_check(ctypes.c_void_p(rec.ctypes.data), 1) == code
    assert field.encode() in lib.wv_last_error(), lib.wv_last_error()
    dst = np.zeros(60 * 24, np.uint8)                                                # the twin runs the same check first
    assert lib.wv_image_size_cpu(ctypes.c_void_p(16), ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(rec.ctypes.data), 1) == code
    assert not dst.any()


def test_check_rejects_scale_overlap_and_count(lib):
    for axis in ("h", "w"):
        rec = base_record()
        rec[0]["src_h"], rec[0]["src_w"], rec[0]["src_row_bytes"] = 700, 700, 2100
        rec[0]["crop_" + axis], rec[0]["res_" + axis] = 651, 10                        # 65.1x; 640 -> 10 passes
        assert lib.wv_image_size_check(ctypes.c_void_p(rec.ctypes.data), 1) == -95
        assert ("crop_" + axis).encode() in lib.wv_last_error() and b"64" in lib.wv_last_error()
        rec[0]["crop_" + axis] = 640
        assert lib.wv_image_size_check(ctypes.c_void_p(rec.ctypes.data), 1) == 0
    two = np.concatenate([base_record(), base_record()])
    two[1]["dst_offset"] = 60 * 24 - 1                                               # one byte into the first destination
    assert lib.wv_image_size_check(ctypes.c_void_p(two.ctypes.data), 2) == -22 and b"dst_offset" in lib.wv_last_error()
    two[1]["dst_offset"] = 60 * 24
    assert lib.wv_image_size_check(ctypes.c_void_p(two.ctypes.data), 2) == 0
    assert lib.wv_image_size_check(None, -1) == -22 and b"n = -1" in lib.wv_last_error()
    assert lib.wv_image_size_check(None, 0) == 0
    assert lib.wv_image_size_check(None, 1) == -22 and b"stages" in lib.wv_last_error()
    assert lib.wv_image_size(None, None, None, 0, 1, 1, 1, None) == 0                # nothing to do: no launch, no GPU needed
    one_ = ctypes.c_void_p(16)
    assert lib.wv_image_size(one_, one_, one_, 1, 224, 224, 259, None) == -95 and b"max_ksize" in lib.wv_last_error()
    assert lib.wv_image_size(one_, one_, one_, 1, 0, 224, 5, None) == -22 and b"max_out_h" in lib.wv_last_error()


def test_host_twin_over_a_ragged_batch_under_asan_and_ubsan(lib, tmp_path):
    """The twin and a stand-alone driver (tests/native/image_size_asan.cpp) compiled with -fsanitize=address,undefined, run as
    a child process: images and outputs back to back in heap blocks of the exact size -- ragged offsets are where an
    off-by-one reads or writes out of bounds.  1-pixel sides, an overhanging window, a crop touching the last row and column."""
    cases = C.ragged_cases()[:-4]                                                    # the small images of the ragged batch
    px = C.image(1, 1, "noise", 4)
    col, row = C.image(1, 9, "noise", 5), C.image(11, 1, "binary", 6)
    cases += [(px, C.stage(px, (5, 3), C.BICUBIC)), (col, C.stage(col, (1, 4), C.BILINEAR)), (col, C.stage(col, (3, 1), C.BICUBIC)),
              (row, C.stage(row, (4, 2), C.BILINEAR, window=(-1, -1, 6, 4), flip=1)),
              (row, C.stage(row, (1, 1), C.BICUBIC, crop=(10, 0, 1, 1)))]
    src, rec, dst_bytes, outs = C.pack(cases, DT)
    exe, fin, fout = tmp_path / "image_size_asan", tmp_path / "in.bin", tmp_path / "out.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "image_size_asan.cpp"),
                           os.path.join(ROOT, "image-retrieval-wavelet_amd", "csrc", "host_image_size.cpp")])
    with open(fin, "wb") as f:
        f.write(np.array([len(rec), src.size, dst_bytes], np.int64).tobytes() + rec.tobytes() + src.tobytes())
    res = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "image_size_asan ok" in res.stdout, res.stderr[-3000:]
    dst = np.fromfile(fout, np.uint8)
    for i, ((arr, st), got) in enumerate(zip(cases, C.unpack(dst, outs))):
        assert np.array_equal(got, C.pillow_stage(arr, st)), (i, st)
