"""PromptedSharedDinoHashing on the GPU against the reference's fixture (tests/golden/prompted_golden.npz): eval through the
grouped LayerNorm kernel, the fused head and the HIP tail, in fp32 and under bf16 autocast; one gradient-cached train step
whose first pass takes the kernel and whose second pass takes stock PyTorch; raw batches through the bound transform."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import prompted_cases as PC
from wvhash import synth
from wvhash.engine.train_step import train_step
from wvhash.models import MultiDomainLayerNorm, PromptedSharedDinoHashing, hash_tail
from wvhash.models.vit import tiny_vit
from wvhash.transforms import SWTTransform, swt2d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prompted_golden.npz"))


def build(name):
    _, _, _, build_seed, state_seed = PC.CASES[name]
    torch.manual_seed(build_seed)
    model = PromptedSharedDinoHashing(backbone=tiny_vit(PC.EMBED, img_size=PC.IMG), **PC.model_kwargs(name))
    return synth.randomize_module(model, state_seed).cuda()


def dsln_modules(model):
    return [m for m in model.modules() if isinstance(m, MultiDomainLayerNorm)]


def library_eval(model, x):
    """Eval without gradients: kernel norms, fused head, HIP tail -> (codes of forward(), logits of the same tail)."""
    with torch.no_grad():
        codes = model(x)
        logits = hash_tail(model.fused_embedding(x), model.hash_fc, model.bn, want=("logits",))["logits"]
    return codes.cpu(), logits.cpu()


def stock_logits(model, x):
    """The same model as stock PyTorch throughout: with gradients enabled every module takes its reference steps."""
    tap = PC.LogitTap(model)
    with torch.enable_grad():
        model(x)
    tap.close()
    return tap.logits.float().cpu()


@pytest.mark.parametrize("name", list(PC.CASES))
def test_eval_matches_the_fixture(name, golden):
    model = build(name).eval()
    x = PC.make_input().cuda()
    want = torch.from_numpy(golden[f"{name}/eval_codes"]).float()
    ref_logits = torch.from_numpy(golden[f"{name}/eval_logits"])
    compared = ~PC.exempt_mask(ref_logits, float(golden[f"{name}/d64"][0]))
    codes, logits = library_eval(model, x)
    print(f"{name}: max |logits - reference| {float((logits - ref_logits).abs().max()):.3e}, compared {int(compared.sum())} of {compared.numel()}")
    assert set(codes.unique().tolist()) <= {-1.0, 1.0}
    assert torch.equal(codes[compared], want[compared])
    assert torch.equal(codes, torch.sign(logits))
    use_dsln = PC.CASES[name][0]
    mods = dsln_modules(model)
    assert len(mods) == (5 if use_dsln else 0)
    assert all(m.kernel_calls == 2 and m.stock_calls == 0 for m in mods)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_eval_under_bf16_autocast_matches_the_stock_autocast_run(name):
    """Exempt bits come from the stock autocast run's own logits: d = how far they are from the stock fp32 logits."""
    for_stock = build(name).eval()
    for p in for_stock.parameters():
        p.requires_grad_(True)                                  # every module then needs gradients: none takes the library
    model = build(name).eval()
    x = PC.make_input().cuda()
    full = stock_logits(for_stock, x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        stock = stock_logits(for_stock, x)
        codes, logits = library_eval(model, x)
    assert all(m.kernel_calls == 0 for m in dsln_modules(for_stock))
    d = float((stock - full).abs().max())
    compared = ~PC.exempt_mask(stock, d)
    print(f"{name}: d {d:.3e}, compared {int(compared.sum())} of {compared.numel()}, "
          f"max |library - stock| under autocast {float((logits.float() - stock).abs().max()):.3e}")
    assert torch.equal(codes[compared], torch.sign(stock)[compared])
    mods = dsln_modules(model)
    assert all(m.kernel_calls == 2 and m.stock_calls == 0 for m in mods)


def test_block_norms_emit_bf16_under_autocast_and_the_final_norm_does_not():
    model = build("dsln_p10").eval()
    seen = {}
    bb = model.shared_backbone
    for label, mod in (("norm1", bb.blocks[0].norm1), ("norm2", bb.blocks[1].norm2), ("norm", bb.norm)):
        mod.register_forward_hook(lambda m, a, out, label=label: seen.setdefault(label, []).append(out.dtype))
    x = PC.make_input().cuda()
    with torch.no_grad():
        model(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model(x)
    assert seen == {"norm1": [torch.float32, torch.bfloat16], "norm2": [torch.float32, torch.bfloat16],
                    "norm": [torch.float32, torch.float32]}


class _SquareLoss(nn.Module):
    takes_embeddings = True

    def forward(self, emb, labels):
        return (emb.float() ** 2).mean(dim=1)


def test_train_step_with_sub_batch_takes_the_kernel_then_stock():
    model = build("dsln_p10").train()
    mods = dsln_modules(model)
    assert len(mods) == 5
    before = model.prompts.detach().clone()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.1)
    x = PC.make_input().cuda()
    labels = torch.arange(5).cuda()
    logs = train_step(model, x, labels, [(_SquareLoss(), 1.0)], [opt], autocast_dtype=torch.bfloat16, sub_batch=2)
    assert np.isfinite(logs["total_loss"])
    # 5 samples in micro-batches of 2: (0, 2) and (2, 5).  Pass 1 (no graph): the kernel; pass 2 (with graph): stock PyTorch
    assert all((m.kernel_calls, m.stock_calls) == (2, 2) for m in mods), [(m.kernel_calls, m.stock_calls) for m in mods]
    assert not torch.equal(model.prompts.detach(), before)       # the step reached the prompts through the backbone


def test_raw_batches_go_through_the_bound_transform():
    model = build("dsln_p1").eval().bind_transform(SWTTransform(level=1, wavelet="haar", defer=True))
    raw = torch.from_numpy(synth.natural_images(3, PC.IMG, PC.IMG, seed=2)).permute(0, 3, 1, 2).contiguous().cuda()
    with torch.no_grad():
        assert torch.equal(model(raw), model(swt2d(raw, "haar", 1)))
