"""Colour jitter on the host (no GPU): wv_colour_jitter_cpu against the live Pillow's ImageEnhance, bit for bit; the
ColorJitter step and the recorder of build_transform(..., sizing="device") against the PIL pipeline of sizing="host"; the
argument check field by field.  Every comparison is exact uint8 equality."""
import ctypes
import os

import numpy as np
import PIL
import pytest
import torch
from PIL import Image, ImageEnhance

import colour_cases as C
from wvhash import _lib
from wvhash.transforms import ColorJitter, build_transform, pil_ops, sizing, size_images_host

DT = sizing.COLOUR_DTYPE
B, CO, S = C.BRIGHTNESS, C.CONTRAST, C.SATURATION


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def one(lib, arr, chain):
    buf, rec = C.run_cpu(lib, [(arr, chain)], DT)
    return C.unpack(buf, rec)[0]


# ---- the nodes that did not build -----------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["host", "device"])
def test_voc_train_node_builds(how):
    tf = build_transform(C.voc_node(), defer=True, sizing=how)
    jitter = [t for t in tf.transforms if type(t).__name__ == "ColorJitter"]
    assert len(jitter) == 1
    if how == "device":                                   # always this package's class: it knows how to record
        assert isinstance(jitter[0], pil_ops.ColorJitter)
        assert jitter[0].brightness == jitter[0].contrast == jitter[0].saturation == (0.75, 1.25) and jitter[0].hue is None


# ---- the twin against Pillow ----------------------------------------------------------------------------------------

def test_ragged_buffer_equals_pillow_and_keeps_the_gaps(lib):
    cases = C.ragged_cases()
    assert {c[0].shape[1] for c in cases} == set(C.WIDTHS) and {c[0].shape[0] for c in cases} == set(C.HEIGHTS)
    assert {tuple(k for k, _ in c[1]) for c in cases} == set(C.orders()) and len(C.orders()) == 16
    used = {f for c in cases for _, f in c[1]}
    assert set(C.FIXED_FACTORS) <= used and any(f not in C.FIXED_FACTORS and 0.75 <= f <= 1.25 for f in used)
    buf, rec = C.run_cpu(lib, cases, DT)
    assert {int(o) % 4 for o in rec["offset"]} == {0, 1, 2, 3} and (rec["row_bytes"] > 3 * rec["w"]).any()
    for i, (got, case) in enumerate(zip(C.unpack(buf, rec), cases)):
        assert np.array_equal(got, C.pillow_chain(case[0], case[1])), (i, case[0].shape, case[1])
    assert np.array_equal(buf, C.pillow_buffer(cases, DT))                           # ... and every byte between the images


@pytest.mark.parametrize("kind", [S, B])
def test_every_colour_equals_pillow(lib, kind):
    arr = C.all_colours()
    flat = arr.reshape(-1, 3).astype(np.uint32)
    assert np.array_equal(flat[:, 0] | flat[:, 1] << 8 | flat[:, 2] << 16, np.arange(1 << 24, dtype=np.uint32))   # each once
    for f in (0.75, 1.25, C.seeded_factor(11)):
        got = one(lib, arr, [(kind, f)])
        assert np.array_equal(got, C.pillow_chain(arr, [(kind, f)])), (kind, f)


def test_contrast_mean_rounds_like_pillow(lib):
    for arr in C.mean_edge_images():
        means = [int(arr[..., 0].astype(np.float64).mean() + 0.5)]
        got = one(lib, arr, [(CO, 0.0)])                                               # factor 0: every byte becomes the mean
        assert np.array_equal(got, C.pillow_chain(arr, [(CO, 0.0)])) and set(np.unique(got)) == set(means), arr.shape
        for f in (0.75, 1.25):
            assert np.array_equal(one(lib, arr, [(CO, f)]), C.pillow_chain(arr, [(CO, f)])), (arr.shape, f)
    assert np.unique(one(lib, C.grey_row([10, 11]), [(CO, 0.0)])).tolist() == [11]    # 10.5 rounds up


def test_contrast_sees_the_image_as_it_is_at_its_place_in_the_chain(lib):
    arr = C.image(53, 37, 21)
    before = [(B, 1.25), (CO, 0.75)]
    after = [(CO, 0.75), (B, 1.25)]
    a, b = one(lib, arr, before), one(lib, arr, after)
    assert not np.array_equal(a, b)
    assert np.array_equal(a, C.pillow_chain(arr, before)) and np.array_equal(b, C.pillow_chain(arr, after))


def test_contrast_sum_above_32_bits(lib):
    arr = np.full((4200, 4200, 3), 255, np.uint8)
    assert 255 * 4200 * 4200 > 1 << 32
    got = one(lib, arr, [(CO, 0.75)])
    ref = np.array(ImageEnhance.Contrast(Image.fromarray(arr)).enhance(0.75))
    assert np.array_equal(got, ref) and int(got.min()) == 255


def test_golden_pins_the_pillow_version_that_wrote_it(lib, golden_dir):
    g = np.load(os.path.join(golden_dir, "colour_golden.npz"))
    assert int(g["n"]) == len(C.golden_cases())
    for i in range(int(g["n"])):
        arr, chain = g[f"in_{i}"], [(int(k), float(f)) for k, f in zip(g[f"kind_{i}"], g[f"factor_{i}"])]
        live, stored = C.pillow_chain(arr, chain), g[f"out_{i}"]
        assert np.array_equal(live, stored), (
            f"Pillow changed: Pillow {PIL.__version__} no longer reproduces case {i} as Pillow {g['pillow_version']} "
            "enhanced it; the library reproduces the stored version's arithmetic")
        assert np.array_equal(one(lib, arr, chain), stored), i


# ---- the argument check -----------------------------------------------------------------------------------------------

def good_records():
    rec = np.zeros(2, dtype=DT)
    rec["offset"], rec["h"], rec["w"], rec["row_bytes"], rec["n_ops"] = [0, 200], 4, 5, 16, 3
    rec["kind"], rec["factor"] = [B, CO, S], [0.75, 1.0, 1.25]
    return rec


def check(lib, rec, n=None):
    rc = lib.wv_colour_jitter_check(ctypes.c_void_p(rec.ctypes.data), len(rec) if n is None else n)
    return rc, lib.wv_last_error().decode()


def test_argument_check_names_the_field(lib):
    assert check(lib, good_records())[0] == 0

    def broken(field, value, index=None):
        rec = good_records()
        if index is None:
            rec[field][1] = value
        else:
            rec[field][1][index] = value
        return check(lib, rec)

    for field, value, index, code, words in (
            ("h", 0, None, -22, "image 1: h = 0"), ("w", -3, None, -22, "image 1: w = -3"),
            ("row_bytes", 14, None, -22, "row_bytes = 14"), ("offset", -1, None, -22, "offset = -1"),
            ("kind", 3, 1, -22, "kind[1] = 3"), ("kind", -1, 0, -22, "kind[0] = -1"),
            ("kind", B, 2, -22, "kind[2] = 0 is listed twice"),
            ("n_ops", 4, None, -22, "n_ops = 4"), ("n_ops", -1, None, -22, "n_ops = -1"),
            ("factor", -0.5, 0, -22, "factor[0] = -0.5"), ("factor", np.inf, 2, -22, "factor[2] = inf"),
            ("factor", np.nan, 1, -22, "factor[1] = nan"),
            ("offset", 62, None, -22, "offset = 62 lies inside image 0"),
            ("h", 16385, None, -95, "h = 16385"), ("w", 16385, None, -95, "w = 16385")):
        if field == "w" and value > 5:
            rec = good_records()
            rec["w"][1], rec["row_bytes"][1] = value, 3 * value
            rc, msg = check(lib, rec)
        else:
            rc, msg = broken(field, value, index)
        assert rc == code and words in msg, (field, value, rc, msg)
    rec = good_records()
    rec["offset"][1] = 63                                                              # image 0 ends at 3 * 16 + 15 = 63
    assert check(lib, rec)[0] == 0
    rec["kind"][1][2], rec["factor"][1][2], rec["n_ops"][1] = 7, -1.0, 2               # beyond n_ops: not looked at
    assert check(lib, rec)[0] == 0
    assert check(lib, rec, n=-1)[0] == -22 and check(lib, rec, n=0)[0] == 0
    # the twin runs the check itself and touches nothing when it fails
    buf = np.full(400, 0xAB, np.uint8)
    rec = good_records()
    rec["kind"][1][1] = B
    assert lib.wv_colour_jitter_cpu(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(rec.ctypes.data), 2) == -22
    assert (buf == 0xAB).all()
    assert lib.wv_colour_jitter_workspace_bytes(5) == 40 and lib.wv_colour_jitter_workspace_bytes(0) == 0


# ---- the Python surface -----------------------------------------------------------------------------------------------

def test_constructor_ranges_and_errors():
    j = ColorJitter(0.25, 0.25, 0.25, 0)
    assert j.brightness == j.contrast == j.saturation == (0.75, 1.25) and j.hue is None
    j = ColorJitter(brightness=1.5, contrast=(0.5, 2), saturation=[1, 1], hue=0.1)
    assert j.brightness == (0.0, 2.5) and j.contrast == (0.5, 2.0) and j.saturation is None and j.hue == (-0.1, 0.1)
    assert ColorJitter(hue=(-0.5, 0.25)).hue == (-0.5, 0.25) and ColorJitter(hue=(0, 0)).hue is None
    assert ColorJitter().brightness is None and ColorJitter(brightness=0).brightness is None
    for bad in ({"brightness": -0.1}, {"contrast": (1.2, 0.8)}, {"saturation": (-0.5, 1)}, {"hue": 0.6}, {"hue": (-0.6, 0)},
                {"hue": -0.1}):
        with pytest.raises(ValueError):
            ColorJitter(**bad)
    for bad in ({"brightness": "much"}, {"contrast": (1, 2, 3)}):
        with pytest.raises(TypeError):
            ColorJitter(**bad)


def expected_draws(seed, ranges):
    """The stated sequence: randperm(4), then one uniform_ per range that is on, brightness, contrast, saturation, hue."""
    torch.manual_seed(seed)
    perm = torch.randperm(4).tolist()
    drawn = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in ranges]
    return [(ColorJitter.KINDS[i], drawn[i]) for i in perm if drawn[i] is not None]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_draw_order(seed):
    img = Image.fromarray(C.image(9, 7, 1))
    j = ColorJitter(0.25, 0.25, 0.25, 0)
    want = expected_draws(seed, (j.brightness, j.contrast, j.saturation, j.hue))
    assert len(want) == 3
    torch.manual_seed(seed)
    lazy = j(sizing.LazyImage(img))
    assert lazy.ops == [("colour", k, f) for k, f in want]
    j = ColorJitter(brightness=0, contrast=(0.5, 1.5), saturation=0, hue=0.2)         # absent operations draw nothing
    want = expected_draws(seed, (None, j.contrast, None, j.hue))
    torch.manual_seed(seed)
    assert j(sizing.LazyImage(img)).ops == [("colour", k, f) for k, f in want] and len(want) == 2
    torch.manual_seed(seed)                                                            # a PIL image: the same draws, applied
    ref = img
    for k, f in expected_draws(seed, (None, j.contrast, None, j.hue)):
        ref = sizing.pil_colour(ref, k, f)
    torch.manual_seed(seed)
    assert np.array_equal(np.array(j(img)), np.array(ref))


def stated_hue(img, factor):
    h, s, v = img.convert("HSV").split()
    h = Image.fromarray(((np.array(h).astype(np.int64) + (int(factor * 255) & 0xFF)) % 256).astype(np.uint8))
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def test_hue_on_the_host_is_the_stated_pil_rule():
    img = Image.fromarray(C.image(31, 17, 2))
    for f in (-0.5, -0.1, 0.0, 0.013, 0.3, 0.5):
        assert np.array_equal(np.array(sizing.pil_colour(img, "hue", f)), np.array(stated_hue(img, f))), f
    assert not np.array_equal(np.array(sizing.pil_colour(img, "hue", 0.3)), np.array(img))
    torch.manual_seed(4)
    drawn = expected_draws(4, (None, None, None, (-0.4, 0.4)))[0][1]
    torch.manual_seed(4)
    assert np.array_equal(np.array(ColorJitter(hue=0.4)(img)), np.array(stated_hue(img, drawn)))
    grey = img.convert("L")
    assert sizing.pil_colour(grey, "hue", 0.2) is grey
    with pytest.raises(ValueError):
        sizing.pil_colour(img, "hue", 0.6)


def test_a_hue_draw_sends_the_image_down_the_pil_fallback():
    node = dict(C.VOC_TRAIN, ColorJitter={"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0.1},
                SWTTransform={"level": 1, "wavelet": "haar"})
    img = Image.fromarray(C.image(200, 180, 3))
    torch.manual_seed(9)
    host = build_transform(node, defer=True)(img)
    torch.manual_seed(9)
    item = build_transform(node, defer=True, sizing="device")(img)
    assert len(item.stages) == 0 and item.colour is None
    assert torch.equal(item.pixels, host.permute(1, 2, 0))
    assert torch.equal(size_images_host(sizing.raw_collate([item]))[0], host.permute(1, 2, 0))


# ---- the stage rule ---------------------------------------------------------------------------------------------------

def lazy_pipelines():
    """name -> (LazyImage after the calls, expected stage count, expected chain lengths per stage)"""
    img = Image.fromarray(C.image(61, 45, 4))
    z = sizing.LazyImage(img)
    chain = lambda im, fs=(1.25, 0.75, 1.1): im.colour("contrast", fs[0]).colour("brightness", fs[1]).colour("saturation", fs[2])
    return {
        "colour then mirror": (chain(z.resize((30, 22), Image.BILINEAR)).transpose(Image.FLIP_LEFT_RIGHT), 1, [3]),
        "mirror then colour": (chain(z.resize((30, 22), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT)), 1, [3]),
        "colour then crop": (chain(z.resize((30, 22), Image.BILINEAR)).crop((3, 2, 20, 19)), 2, [3, 0]),
        "colour then padded crop": (chain(z.resize((30, 22), Image.BILINEAR)).crop((-3, -2, 33, 19)), 2, [3, 0]),
        "colour then resample": (chain(z.crop((5, 4, 45, 40))).resize((24, 20), Image.BICUBIC), 2, [3, 0]),
        "colour on a padded window": (chain(z.resize((30, 22), Image.BILINEAR).crop((-4, -3, 36, 30))), 1, [3]),
        "colour before any geometry": (chain(z).resize((30, 22), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT), 2, [3, 0]),
        "colour alone": (chain(z), 1, [3]),
        "two jitters": (chain(chain(z.resize((30, 22), Image.BILINEAR)).crop((3, 2, 20, 19)), (0.8, 1.2, 0.9)), 2, [3, 3]),
        "two jitters that share a stage": (z.resize((30, 22), Image.BILINEAR).colour("brightness", 1.2).colour("contrast", 0.8), 1, [2]),
    }


@pytest.mark.parametrize("name", sorted(lazy_pipelines()))
def test_stage_rule(name):
    lazy, n_stages, chains = lazy_pipelines()[name]
    stages = sizing.stages_from_ops(61, 45, lazy.ops)
    assert len(stages) == n_stages and [len(st["colour"]) for st in stages] == chains
    item = lazy.to_item()
    assert len(item.stages) == n_stages and item.colour["n_ops"].tolist() == chains
    rb = sizing.raw_collate([item])
    assert [c[1] for c in rb.colour_launches] == [1 if c else 0 for c in chains]
    assert np.array_equal(size_images_host(rb)[0].numpy(), np.array(lazy.materialize()))


def test_a_second_operation_of_a_kind_on_one_stage_falls_back_to_pil():
    z = sizing.LazyImage(Image.fromarray(C.image(61, 45, 4))).resize((30, 22), Image.BILINEAR)
    twice = z.colour("brightness", 1.2).colour("contrast", 0.8).colour("brightness", 0.9)
    with pytest.raises(sizing.NotRecordable):
        sizing.stages_from_ops(61, 45, twice.ops)
    item = twice.to_item()
    assert len(item.stages) == 0 and item.colour is None
    assert np.array_equal(item.pixels.numpy(), np.array(twice.materialize()))
    with pytest.raises(ValueError):
        z.colour("gamma", 1.0)


def test_raw_batch_keeps_its_positional_constructor_and_moves_the_colour_records():
    rb = sizing.RawBatch(torch.zeros(4, dtype=torch.uint8), torch.zeros(1, 20, dtype=torch.int32), [(0, 1, 1, 1, 1)], (1, 1, 1), 16)
    assert rb.colour is None and rb.colour_launches == () and rb.to("cpu").colour is None
    it = sizing.RawItem(torch.zeros(1, 1, 3, dtype=torch.uint8), np.zeros(0, sizing.STAGE_DTYPE))
    assert it.colour is None and it.out_hw == (1, 1)
    lazy = sizing.LazyImage(Image.fromarray(C.image(9, 7, 1))).colour("contrast", 0.8)
    rb = sizing.raw_collate([lazy.to_item()])
    moved = rb.to("cpu")
    assert moved.colour_launches == rb.colour_launches == ((0, 1, 7, 9),) and torch.equal(moved.colour, rb.colour)
    assert rb.colour.dtype == torch.int32 and tuple(rb.colour.shape) == (1, 12)


# ---- end to end on the host -------------------------------------------------------------------------------------------

def test_voc_train_node_device_items_equal_the_host_batch():
    imgs = [Image.fromarray(C.image(*C.SIZES[i % 3], 60 + i)) for i in range(5)]
    torch.manual_seed(5)
    th = build_transform(C.voc_node(), defer=True)
    host = torch.stack([th(im) for im in imgs])
    torch.manual_seed(5)
    td = build_transform(C.voc_node(), defer=True, sizing="device")
    items = [td(im) for im in imgs]
    assert all(len(it.stages) == 2 and it.colour["n_ops"].tolist() == [0, 3] for it in items)
    rb = sizing.raw_collate(items)
    assert rb.colour_launches == ((0, 0, 0, 0), (0, 5, 224, 224))
    assert torch.equal(size_images_host(rb), host.permute(0, 2, 3, 1))
