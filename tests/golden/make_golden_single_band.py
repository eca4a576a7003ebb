#!/usr/bin/env python3
"""Regenerates tests/golden/single_band_golden.npz.  Run in the BUILD container only (needs /root/reference):
    python tests/golden/make_golden_single_band.py

What it pins: the REFERENCE's own SingleBandNet / DetailTesterNet (main/models/detail_tester.py) and DINOHashBaseline
(main/models/dino_baseline.py), imported by file path as make_golden.py imports the fusion heads.  `timm` is absent here, so
a stub module stands in for the import and the isinstance check of DetailTesterNet.forward; `load_dinov2` (torch.hub) is
replaced by the tiny seeded backbone of tests/single_band_cases.py.  Per case (single_band_cases.CASES): the model is built
under a fixed seed, its BatchNorm statistics and affine parameters and its projection are given non-trivial seeded values,
and the fixture stores that state dict, the output of a training-mode forward on the shared [5, 3, 4, 16, 16] input, and
-- from the stored state again -- the eval-mode output.

Fixtures are data only (tensors).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import single_band_cases as SB  # noqa: E402

REF = "/root/reference"


def load_reference_models():
    timm = types.ModuleType("timm")
    timm.models = types.ModuleType("timm.models")
    timm.models.resnet = types.ModuleType("timm.models.resnet")
    timm.models.resnet.ResNet = type("ResNet", (torch.nn.Module,), {})
    sys.modules.update({"timm": timm, "timm.models": timm.models, "timm.models.resnet": timm.models.resnet})
    pkg = types.ModuleType("refmodels")
    pkg.__path__ = [os.path.join(REF, "main", "models")]
    sys.modules["refmodels"] = pkg
    mods = {}
    for name in ("hub_utils", "detail_tester", "dino_baseline"):
        spec = importlib.util.spec_from_file_location(f"refmodels.{name}", os.path.join(REF, "main", "models", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refmodels.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    for name in ("detail_tester", "dino_baseline"):
        mods[name].load_dinov2 = lambda *a, **k: SB.TinyBackbone()
    return {"SingleBandNet": mods["detail_tester"].SingleBandNet, "DetailTesterNet": mods["detail_tester"].DetailTesterNet,
            "DINOHashBaseline": mods["dino_baseline"].DINOHashBaseline}


def make():
    classes = load_reference_models()
    g = torch.Generator().manual_seed(2024)
    x5 = torch.randn(*SB.INPUT_SHAPE, generator=g)
    out = {"input": x5.numpy()}
    for i, (name, (cls, kwargs)) in enumerate(SB.CASES.items()):
        torch.manual_seed(100 + i)
        model = classes[cls](**kwargs)
        with torch.no_grad():
            for mod in model.modules():
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.running_mean.copy_(0.3 * torch.randn(mod.num_features))
                    mod.running_var.copy_(0.5 + torch.rand(mod.num_features))
                    mod.weight.copy_(0.5 + torch.rand(mod.num_features))
                    mod.bias.copy_(0.2 * torch.randn(mod.num_features))
                elif isinstance(mod, torch.nn.Linear) and mod is not model.backbone.proj:
                    mod.weight.copy_(0.05 * torch.randn_like(mod.weight))
                    if mod.bias is not None:
                        mod.bias.copy_(0.1 * torch.randn_like(mod.bias))
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        xin = SB.model_input(name, x5)
        train_out = model.train()(xin).detach()
        model.load_state_dict(state, strict=True)
        with torch.no_grad():
            eval_out = model.eval()(xin)
        if cls != "SingleBandNet" or kwargs["is_hashing"]:
            assert set(eval_out.unique().tolist()) <= {-1.0, 1.0}
        for k, v in state.items():
            out[f"{name}/state/{k}"] = v.numpy()
        out[f"{name}/train_out"] = train_out.numpy()
        out[f"{name}/eval_out"] = eval_out.numpy()
        print(f"{name}: {cls} keys {sorted(state)[:3]}... train {tuple(train_out.shape)} eval mean {float(eval_out.mean()):+.3f}")
    path = os.path.join(HERE, "single_band_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    make()
