"""SingleBandNet, DINOHashBaseline and DetailTesterNet against the reference's own modules (no GPU):
tests/golden/single_band_golden.npz holds, per case of single_band_cases.CASES, the state dict of the reference's model
(tiny seeded backbone in place of torch.hub's), the shared [5, 3, 4, 16, 16] input and the outputs in train and eval mode."""
import os

import numpy as np
import pytest
import torch

import single_band_cases as SB
import wvhash.models
from wvhash.transforms import SWTTransform

# config/model/{single_band,dino_hashing,baseline_vits_hash,detail_tester}.yaml of the reference: name, kwargs (unchanged)
YAML = {
    "single_band": ("SingleBandNet", dict(backbone_name="dinov2_vits14", detail_index=0, output_dim=384, with_autocast=True,
                                          is_hashing=False)),
    "dino_hashing": ("DINOHashBaseline", dict(dino_backbone="dinov2_vits14", embed_dim=384, binary_config={"nbits": 64},
                                              with_autocast=True)),
    "baseline_vits_hash": ("DINOHashBaseline", dict(dino_backbone="dinov2_vits14", embed_dim=384, binary_config={"nbits": 64},
                                                    with_autocast=False)),
    "detail_tester": ("DetailTesterNet", dict(backbone_name="dinov2_vits14", detail_index=0, output_dim=64, with_autocast=True)),
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "single_band_golden.npz"))


def build(name, golden):
    cls, kwargs = SB.CASES[name]
    model = getattr(wvhash.models, cls)(backbone=SB.TinyBackbone(seed=99), **kwargs)    # the state dict overwrites the seed
    model.load_state_dict(SB.load_state(golden, name), strict=True)
    return model


@pytest.mark.parametrize("name", list(SB.CASES))
def test_reference_state_loads_strictly_and_train_output_matches(name, golden):
    model = build(name, golden).train()
    x = SB.model_input(name, torch.from_numpy(golden["input"]))
    got = model(x).detach()
    want = torch.from_numpy(golden[f"{name}/train_out"])
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", list(SB.CASES))
def test_eval_output_matches_through_the_host_twin(name, golden):
    model = build(name, golden).eval()
    model.host_twin = True                          # hashing tails: the library's wv_hash_tail_cpu; the rest stock PyTorch
    x = SB.model_input(name, torch.from_numpy(golden["input"]))
    with torch.no_grad():
        got = model(x)
    want = torch.from_numpy(golden[f"{name}/eval_out"])
    cls, kwargs = SB.CASES[name]
    if cls == "SingleBandNet" and not kwargs["is_hashing"]:
        assert float((got - want).abs().max()) <= 1e-6          # L2-normalised embedding
    else:
        assert torch.equal(got, want)                           # codes
        model.host_twin = False
        with torch.no_grad():
            assert torch.equal(model(x), want)                  # ... and stock PyTorch on the host without the switch


def test_hashing_tails_take_the_library_path(golden, monkeypatch):
    """Eval, no grad, host_twin: SingleBandNet (is_hashing) and DINOHashBaseline call hash_tail; DetailTesterNet never."""
    import wvhash.models.single_band as M
    calls = []
    real = M.hash_tail
    monkeypatch.setattr(M, "hash_tail", lambda *a, **k: calls.append(k.get("host_twin")) or real(*a, **k))
    x5 = torch.from_numpy(golden["input"])
    for name, expect in (("sb_hash_bn_d1", 1), ("sb_hash_nobn_d2", 1), ("dino_baseline", 1), ("sb_embed_d0", 0),
                         ("detail_tester_d1", 0)):
        model = build(name, golden).eval()
        model.host_twin = True
        del calls[:]
        with torch.no_grad():
            model(SB.model_input(name, x5))
        assert calls == [True] * expect, name
        del calls[:]
        model(SB.model_input(name, x5))                          # under grad: stock PyTorch
        model.train()(SB.model_input(name, x5))
        assert calls == [], name


@pytest.mark.parametrize("yaml", list(YAML))
def test_names_resolve_with_the_reference_yaml_kwargs(yaml):
    cls, kwargs = YAML[yaml]
    model = getattr(wvhash.models, cls)(backbone=SB.TinyBackbone(), **kwargs)
    keys = set(k.split(".")[0] for k in model.state_dict())
    assert keys == {"SingleBandNet": {"backbone"}, "DINOHashBaseline": {"backbone", "hash_head"},
                    "DetailTesterNet": {"backbone", "bn", "hash_fc"}}[cls]
    if cls == "SingleBandNet":
        assert isinstance(model.head, torch.nn.Identity) and isinstance(model.bn, torch.nn.Identity)


def test_state_dict_keys_of_the_hashing_variants():
    net = wvhash.models.SingleBandNet(detail_index=1, output_dim=64, is_hashing=True, backbone=SB.TinyBackbone())
    assert net.head.bias is None and {"head.weight", "bn.weight", "bn.running_mean"} <= set(net.state_dict())
    net = wvhash.models.SingleBandNet(detail_index=1, output_dim=64, is_hashing=True, use_bn=False, backbone=SB.TinyBackbone())
    assert net.head.bias is not None and isinstance(net.bn, torch.nn.Identity)
    base = wvhash.models.DINOHashBaseline(backbone=SB.TinyBackbone())
    assert {"hash_head.0.weight", "hash_head.1.weight", "hash_head.1.running_var"} <= set(base.state_dict())
    assert "hash_head.0.bias" not in base.state_dict()


def test_frozen_baseline_keeps_the_backbone_out_of_training():
    base = wvhash.models.DINOHashBaseline(frozen=True, backbone=SB.TinyBackbone())
    assert not any(p.requires_grad for p in base.backbone.parameters())
    base.train()
    assert not base.backbone.training
    out = base(torch.randn(4, 3, 16, 16))
    out.sum().backward()
    assert base.hash_head[0].weight.grad is not None and base.backbone.proj.weight.grad is None
    free = wvhash.models.DINOHashBaseline(frozen=False, backbone=SB.TinyBackbone()).train()
    free(torch.randn(4, 3, 16, 16)).sum().backward()
    assert free.backbone.proj.weight.grad is not None
    with torch.no_grad():
        assert not free(torch.randn(4, 3, 16, 16)).requires_grad


def test_detail_tester_refuses_timm_backbones():
    with pytest.raises(ValueError, match="timm"):
        wvhash.models.DetailTesterNet(backbone_name="resnet50", backbone=SB.TinyBackbone())
    with pytest.raises(ValueError, match="timm"):
        wvhash.models.DetailTesterNet(backbone=SB.TinyBackbone())            # the reference's default is resnet50


def test_raw_batches_need_a_bound_transform():
    raw = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    single = wvhash.models.SingleBandNet(detail_index=1, backbone=SB.TinyBackbone()).eval()
    tester = wvhash.models.DetailTesterNet("dinov2_vits14", backbone=SB.TinyBackbone()).eval()
    for model in (single, tester):
        with pytest.raises(RuntimeError, match="never guessed"):
            model(raw)
    with pytest.raises(RuntimeError, match="never guessed"):
        tester(raw.float())                                                  # DetailTesterNet always slices a band
    # the reference's `if x.dim() == 5`: a float image batch goes to SingleBandNet's backbone as it is
    x = torch.randn(2, 3, 16, 16)
    with torch.no_grad():
        want = torch.nn.functional.normalize(single.backbone(x)["x_norm_clstoken"], p=2, dim=1)
        assert torch.equal(single(x), want)


def test_bound_transform_feeds_the_band_on_the_host():
    """Host tensors take the host twins: a bound deferred SWTTransform gives the codes of the expanded 5-D input."""
    from wvhash.transforms import swt2d_host
    raw = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(4, 3, 16, 24), dtype=np.uint8))
    bands = swt2d_host(raw, "db2", 1)
    for index in range(4):
        net = wvhash.models.SingleBandNet(detail_index=index, output_dim=64, is_hashing=True,
                                          backbone=SB.TinyBackbone()).eval()
        net.bind_transform(SWTTransform(level=1, wavelet="db2", defer=True))
        with torch.no_grad():
            assert torch.equal(net(raw), net(bands))
