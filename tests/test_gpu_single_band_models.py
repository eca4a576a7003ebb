"""The single-band and baseline models on the GPU: a raw uint8 batch through the bound deferred transform (the single-band
kernel for SWTTransform, the generic slice for RawStackTransform) gives the codes of the expanded 5-D input bit for bit;
evaluate() agrees between the deferred and the expanded plugin; packed codes; bf16 bands under autocast."""
import numpy as np
import pytest
import torch
from PIL import Image
from torch.utils.data import Dataset

import single_band_cases as SB
from wvhash import synth
from wvhash.engine import evaluate
from wvhash.engine import hamming as H
from wvhash.models import DINOHashBaseline, SingleBandNet
from wvhash.transforms import RawStackTransform, SWTTransform, rawstack, swt2d

pytestmark = pytest.mark.gpu


def single_band(index, nbits=64):
    torch.manual_seed(index)
    net = SingleBandNet(detail_index=index, output_dim=nbits, is_hashing=True, backbone=SB.TinyBackbone(seed=index))
    net.head.weight.data.mul_(50)                         # spread the logits away from 0
    return net.cuda().eval()


def raw_batch(n=6, h=64, w=48, seed=1):
    return torch.from_numpy(synth.natural_images(n, h, w, seed=seed)).permute(0, 3, 1, 2).contiguous().cuda()


@pytest.mark.parametrize("index", range(4))
def test_deferred_input_gives_the_codes_of_the_expanded_input(index):
    x = raw_batch()                                       # uint8 [6, 3, 64, 48]: a sliding-kernel shape
    net = single_band(index).bind_transform(SWTTransform(level=3, wavelet="db2", defer=True))
    with torch.no_grad():
        got = net(x)
        want = net(swt2d(x, "db2", 3))
        other = net(swt2d(x, "db2", 3)[:, :, (index + 1) % 4].contiguous())
        nhwc = net(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))      # the [B,3,H,W] view of sized [B,H,W,3] images
    assert set(got.unique().tolist()) <= {-1.0, 1.0}
    assert torch.equal(got, want) and torch.equal(nhwc, want)
    assert not torch.equal(got, other)                    # the test can tell the bands apart
    net.bind_transform(RawStackTransform(copies=4, defer=True))                 # the raw4 control arm: the generic path
    with torch.no_grad():
        assert torch.equal(net(x), net(rawstack(x, 4)))


class SynthHashing(Dataset):
    """{"image","label","path"} items like MIRFlickrHashing.__getitem__ (flikr_coco.py:52-63)."""

    def __init__(self, n, seed, transform):
        self.imgs = synth.natural_images(n, 72, 56, seed=seed)
        self.labels = synth.multi_hot_labels(n, 10, 0.3, seed)
        self.transform = transform

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        return {"image": self.transform(Image.fromarray(self.imgs[i])), "label": self.labels[i], "path": str(i)}


def test_evaluate_agrees_between_the_deferred_and_the_expanded_plugin():
    results = []
    for defer in (True, False):
        tf = SWTTransform(level=3, wavelet="db2", defer=defer)
        dts = {"test": SynthHashing(8, 1, tf), "gallery": SynthHashing(16, 2, tf)}
        m = evaluate(single_band(1), test_dataset=dts, epoch=1, batch_size=8, num_workers=0, k=5, distance_metric="hamming",
                     exclude=["mean_reciprocal_rank", "precision_at_1", "r_precision", "rpr", "pr", "pr_rc"])
        results.append(m["test"])
    deferred, expanded = results
    keys = [k for k in expanded if k == "maphashing_level0" or "bit_balance" in k]
    assert "maphashing_level0" in keys and len(keys) >= 2, sorted(expanded)
    for k in keys:
        assert deferred[k] == expanded[k], (k, deferred[k], expanded[k])


def test_encode_packed_equals_packing_the_forward_codes():
    x = raw_batch(9, 56, 56, seed=4).float() / 255.0
    torch.manual_seed(3)
    base = DINOHashBaseline(binary_config={"nbits": 96}, backbone=SB.TinyBackbone(seed=5))
    base.hash_head[0].weight.data.mul_(50)
    base = base.cuda().eval()
    with torch.no_grad():
        codes = base(x)
        assert torch.equal(codes, torch.sign(base.hash_head(base.backbone(x)["x_norm_clstoken"])))   # stock PyTorch tail
        assert torch.equal(base.encode_packed(x), H.pack_codes(codes))
        net = single_band(2, nbits=96).bind_transform(SWTTransform(level=1, wavelet="haar", defer=True))
        raw = raw_batch(5, 40, 40, seed=6)
        assert torch.equal(net.encode_packed(raw), H.pack_codes(net(raw)))


def test_bf16_band_under_autocast():
    seen = []
    net = single_band(3).bind_transform(SWTTransform(level=3, wavelet="db2", defer=True))
    net.backbone.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, tuple(args[0].shape))))
    x = raw_batch()
    with torch.no_grad():
        net(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            net(x)
    assert seen == [(torch.float32, (6, 3, 64, 48)), (torch.bfloat16, (6, 3, 64, 48))]
