"""PromptedSharedDinoHashing and MultiDomainLayerNorm against the reference's own modules (no GPU):
tests/golden/prompted_golden.npz holds, per case of prompted_cases.CASES, the layout and digest of the reference model's
state dict (filled by synth.randomize_module; prompted_cases explains the form), its training-mode output, its eval-mode
logits and codes on the shared [5, 3, 4, 28, 28] input, and what its constructor left of the global random stream."""
import os

import numpy as np
import pytest
import torch

import prompted_cases as PC
import wvhash.models
from wvhash import synth
from wvhash.models import MultiDomainLayerNorm, PromptedSharedDinoHashing
from wvhash.models.vit import tiny_vit


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prompted_golden.npz"))


def build(name, seeded_state=True):
    """Seed, backbone, model -- the order in which the reference's constructor draws -- then the case's state."""
    _, _, _, build_seed, state_seed = PC.CASES[name]
    torch.manual_seed(build_seed)
    model = PromptedSharedDinoHashing(backbone=tiny_vit(PC.EMBED, img_size=PC.IMG), **PC.model_kwargs(name))
    draw = torch.randn(1)
    prompts_init = model.prompts.detach().clone()
    if seeded_state:
        synth.randomize_module(model, state_seed)
    return model, draw, prompts_init


def host_twins(model, norms=True):
    """A model meant to run on the host: the library's host twins for the fusion head and the hash tail, and (`norms`) for the
    grouped LayerNorm -- without it the per-domain norms run the reference's chunk / norm / cat."""
    model.host_twin = model.fusion_head.host_twin = True
    for m in model.modules():
        if isinstance(m, MultiDomainLayerNorm):
            m.host_twin = norms
    return model


def dsln_modules(model):
    return [m for m in model.modules() if isinstance(m, MultiDomainLayerNorm)]


@pytest.mark.parametrize("name", list(PC.CASES))
def test_reference_state_loads_strictly_and_construction_draws_alike(name, golden):
    model, draw, prompts_init = build(name, seeded_state=False)
    keys, shapes = PC.state_layout(model)
    assert list(keys) == list(golden[f"{name}/keys"]) and list(shapes) == list(golden[f"{name}/shapes"])
    ref_shaped = {k: torch.zeros([int(d) for d in s.split(",") if d], dtype=model.state_dict()[k].dtype)
                  for k, s in zip(golden[f"{name}/keys"], golden[f"{name}/shapes"])}
    model.load_state_dict(ref_shaped, strict=True)
    assert torch.equal(draw, torch.from_numpy(golden[f"{name}/rng_after_init"]))           # RNG consumption
    assert torch.equal(prompts_init, torch.from_numpy(golden[f"{name}/prompts_init"]))     # ... and the init itself
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == list(golden[f"{name}/requires_grad"])
    model, _, _ = build(name)
    assert synth.state_sha(model.state_dict()) == str(golden[f"{name}/sha"])               # the reference's values, all of them
    prefix = f"{name}/state/"
    stored = [k for k in golden.files if k.startswith(prefix)]
    assert stored
    for k in stored:
        assert torch.equal(model.state_dict()[k[len(prefix):]], torch.from_numpy(golden[k])), k


@pytest.mark.parametrize("name", list(PC.CASES))
def test_train_output_matches(name, golden):
    model, _, _ = build(name)
    got = model.train()(PC.make_input()).detach()
    want = torch.from_numpy(golden[f"{name}/train_out"])
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-5
    assert all(m.kernel_calls == 0 for m in dsln_modules(model))                  # gradients: stock PyTorch
    frozen = PC.CASES[name][2]
    assert model.shared_backbone.training == (not frozen)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_eval_codes_match_on_the_host(name, golden):
    """Host twins throughout (grouped LayerNorm, fusion head, hash tail), then with the norms as stock PyTorch."""
    want = torch.from_numpy(golden[f"{name}/eval_codes"]).float()
    ref_logits = torch.from_numpy(golden[f"{name}/eval_logits"])
    d64 = float(golden[f"{name}/d64"][0])
    compared = ~PC.exempt_mask(ref_logits, d64)
    assert float(golden["exempt_factor"][0]) == PC.EXEMPT_FACTOR
    assert float((~compared).float().mean()) <= PC.EXEMPT_CAP
    model, _, _ = build(name)
    model.eval()
    x = PC.make_input()
    for twins in (True, False):
        host_twins(model, twins)
        with torch.no_grad():
            got = model(x)
            logits = model.bn(model.hash_fc(model.fused_embedding(x)))
        assert set(got.unique().tolist()) <= {-1.0, 1.0}
        assert torch.equal(got[compared], want[compared]), twins
        assert float((logits - ref_logits).abs().max()) <= PC.EXEMPT_FACTOR * d64, twins
    calls = [m.kernel_calls for m in dsln_modules(model)]
    use_dsln = PC.CASES[name][0]
    assert len(calls) == (5 if use_dsln else 0) and all(c == 2 for c in calls)   # two forwards per round: twins, then stock
    assert all(m.stock_calls == 2 for m in dsln_modules(model))


def test_emit_dtype_is_set_on_the_block_norms_only():
    model, _, _ = build("dsln_p1", seeded_state=False)
    bb = model.shared_backbone
    assert all(blk.norm1.emit_dtype == "auto" and blk.norm2.emit_dtype == "auto" for blk in bb.blocks)
    assert bb.norm.emit_dtype is None                            # the head reads it
    plain, _, _ = build("plain_p1_frozen", seeded_state=False)
    assert not dsln_modules(plain) and not plain.shared_backbone.training
    assert wvhash.models.PromptedSharedDinoHashing is PromptedSharedDinoHashing


@pytest.mark.parametrize("name", list(PC.BARE_CASES))
def test_bare_module_on_sequence_counts_the_domains_do_not_divide(name, golden):
    N, T, E, seed = PC.BARE_CASES[name]
    module = synth.randomize_module(MultiDomainLayerNorm(torch.nn.LayerNorm(E, eps=1e-6), num_domains=4), seed)
    want = torch.from_numpy(golden[f"{name}/out"])
    x = PC.bare_input(name)
    with torch.no_grad():
        assert float((module(x) - want).abs().max()) <= 1e-6     # stock steps
        module.host_twin = True
        assert float((module(x) - want).abs().max()) <= 1e-5     # the library's host twin
    assert (module.stock_calls, module.kernel_calls) == (1, 1)


def test_raw_batches_need_a_bound_transform():
    model, _, _ = build("dsln_p1")
    host_twins(model.eval())
    raw = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(3, 3, PC.IMG, PC.IMG), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="never guessed"):
        model(raw)
