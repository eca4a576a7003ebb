"""The training step of BASELINE configs c2 and c4 on the GPU: raw uint8 batches of a deferred
transform -> batched HIP SWT inside the step (bf16 sub-bands under bf16 autocast) -> stock-PyTorch forward/backward of
the band-attention hashing model with the proxy hashing loss + orthogonality loss -> optimizer step.
Reference: run.py:162-166, main/engine/base_update.py:52-292, main/losses/hash_loss.py:17-59.

And the step against the reference's own step (tests/golden/train_step_golden.npz, made by
tests/golden/make_golden_train_step.py; cases: tests/train_step_cases.py) on the device: every case in fp32, the fused HIP
losses inside the step, the RNG replay under dropout, a raw batch against its expanded input."""
import functools
import os

import numpy as np
import pytest
import torch

import train_step_cases as TS
from wvhash import losses as L
from wvhash import synth
from wvhash.engine import backward_step, make_averager, train_step
from wvhash.losses import HashLoss
from wvhash.models import MultiDinoHashing, SharedDinoHashing
from wvhash.models.vit import tiny_vit
from wvhash.transforms import SWTTransform, swt2d

pytestmark = pytest.mark.gpu


def build(cls, nq, nbits, dropout=0.1, level=1, wavelet="haar"):
    torch.manual_seed(0)
    fusion = {"type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "num_queries": nq, "dropout": dropout,
              "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
    if cls is MultiDinoHashing:
        net = cls([{"name": "dinov2_vits14", "frozen": True}] * 4, fusion, {"nbits": nbits}, backbones=[tiny_vit() for _ in range(4)])
    else:
        net = cls({"name": "dinov2_vits14", "frozen": True}, fusion, {"nbits": nbits}, backbone=tiny_vit())
    for name, p in net.named_parameters():
        if name.endswith(".gamma"):
            p.data.fill_(1.0)
    net = net.cuda().train().bind_transform(SWTTransform(level=level, wavelet=wavelet, defer=True))
    crit = HashLoss(num_classes=38, embedding_size=nbits).cuda()
    return net, [(crit, 1.0)]


def batch(n=16, seed=1):
    x = torch.from_numpy(synth.natural_images(n, 224, 224, seed=seed)).permute(0, 3, 1, 2).contiguous()   # raw uint8
    return x, synth.multi_hot_labels(n, 38, 0.10, seed)


def test_c2_shared_dino_training_steps_on_raw_batches():
    net, criteria = build(SharedDinoHashing, nq=4, nbits=64, level=3, wavelet="db2")
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=2e-3)
    avg = make_averager(net, criteria)                            # world size 1: a no-op, same call as under torchrun
    x, y = batch()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    losses = []
    for _ in range(6):
        logs = train_step(net, x, y, criteria, {"net": opt}, averager=avg, autocast_dtype=torch.bfloat16, clip_grad=5.0)
        assert {"HashLoss", "Ortho_Loss", "total_loss"} <= set(logs) and all(torch.isfinite(torch.tensor(v)) for v in logs.values())
        losses.append(logs["HashLoss"])
    assert losses[-1] < losses[0]                                 # the same batch, six steps: the loss goes down
    after = net.state_dict()
    assert not torch.equal(before["fusion_head.query_tokens"], after["fusion_head.query_tokens"])
    assert not torch.equal(before["hash_fc.weight"], after["hash_fc.weight"])
    assert all(torch.equal(before[k], after[k]) for k in before if k.startswith("shared_backbone"))   # frozen
    assert all(p.grad is None for p in net.shared_backbone.parameters())


def test_gradient_cached_micro_batches_equal_the_single_pass_gradient():
    x, y = batch(12, seed=2)
    grads = []
    for sub in (None, 5):
        net, criteria = build(SharedDinoHashing, nq=4, nbits=64, dropout=0.0)
        net.bn.eval()                                             # the model's own BatchNorm sees micro-batch statistics otherwise
        backward_step(net, x, y, criteria, autocast_dtype=None, sub_batch=sub)
        grads.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and "fusion_head.mlp.0.weight" in grads[0]
    for k in grads[0]:
        assert torch.allclose(grads[0][k], grads[1][k], rtol=2e-3, atol=2e-6), k


def test_c4_multi_dino_bf16_step_feeds_bf16_sub_bands():
    net, criteria = build(MultiDinoHashing, nq=8, nbits=128)
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3)
    x, y = batch(8, seed=3)
    seen = []
    hooks = [b.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, tuple(args[0].shape)))) for b in net.backbones]
    logs = train_step(net, x, y, criteria, [opt], autocast_dtype=torch.bfloat16, sub_batch=4)
    for h in hooks:
        h.remove()
    assert all(dt == torch.bfloat16 and shp[1:] == (3, 224, 224) for dt, shp in seen)   # the kernel wrote bf16 bands
    assert len(seen) == 4 * 2 * 2                                 # 4 backbones x 2 micro-batches x (no-grad pass + replay)
    assert torch.isfinite(torch.tensor(logs["total_loss"]))
    with torch.no_grad():                                          # eval after the step: the HIP head + tail take over
        codes = net.eval()(swt2d(x.cuda(), "haar", 1))
    assert tuple(codes.shape) == (8, 128) and set(codes.unique().tolist()) <= {-1.0, 1.0}


# ---------------------------------------------------------------------------------------------------------------------
# The step on the device against the reference's own step (tests/golden/train_step_golden.npz)
# ---------------------------------------------------------------------------------------------------------------------
# The yardstick is not the code under test: the truth is the same step on the host in float64 (net.double(), double inputs),
# e_ref = how far the fixture -- the reference's own fp32 step -- lies from it (grad_err over the gradients, scalar_err over
# the logged values), and the device may lie 4 x e_ref from the truth, the margin used for the attention maps.
# e_ref itself is held below E_REF_MAX, which ties the truth to the reference (a truth from a wrong step is O(1) away and would
# make the rule vacuous): one fp32 rounding of a score of magnitude nbits = 16 is 1e-6; SupAP / SmoothAP divide score
# differences by tau = 0.01, 1e-4 in the argument of their sigmoids, so the reference's fp32 step can lie about 1e-4 from the
# exact one (base_supap_ids under micro-batches does: 1.5e-4); ten such roundings are allowed.
# Floor under 4 x e_ref for the LOGGED VALUES only, in fp32 epsilons of the value: a logged scalar is one fp32 number, and
# the fixture's happens to lie within 4e-9 of the float64 figure on some cases (base_supap_multi), which no other order of
# evaluation can be asked to meet.  The longest sums of these models have 64 terms (out_proj over Nq * E, mlp.2 over 4 E);
# two fp32 orders of a 64-term sum differ by up to 64 epsilons of its largest partial sum.  The gradients need no floor.
MARGIN = 4.0
FLOOR = 64 * 2.0 ** -23
E_REF_MAX = 1e-3
SETTINGS = [(c, sub) for c in TS.CASES for sub in TS.SUB_BATCHES]
FUSED_SETTINGS = [(c, sub) for c, sub in SETTINGS if any(kind in TS.FUSED_KINDS for kind, _ in c.criteria)]


def _setting_id(p):
    return f"{p[0].name}-{TS.sub_tag(p[1])}"


@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_golden.npz"))


def _proxies(case):
    key = f"{case.name}/proxies"
    return torch.from_numpy(_gold()[key]) if key in _gold().files else None


def _step(case, sub, device, double=False, fused=None, seed=None):
    """backward_step of a case from the fixture's state -> (logs, gradients of the trainable parameters)"""
    net = TS.wvhash_model(case, TS.load_state(_gold(), case))
    criteria = TS.wvhash_criteria(case, _proxies(case))
    x, y = TS.images(case), TS.labels(case)
    if double:
        net, x = net.double(), x.double()
        criteria = [(c.double(), w) for c, w in criteria]
    net = net.to(device)
    criteria = [(c.to(device), w) for c, w in criteria]
    for c, _ in criteria:
        if fused is not None and hasattr(c, "fused"):
            c.fused = fused
    torch.manual_seed(4000 + case.seed if seed is None else seed)
    logs = backward_step(net, x, y, criteria, autocast_dtype=None, sub_batch=sub)
    return logs, {k: p.grad.detach().clone() for k, p in TS.trainable(net).items() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _truth(name, sub):
    """-> (logs, gradients) of the float64 step on the host, and e_ref = (scalar, gradient) error of the fixture against it"""
    case, gold, tag = TS.BY_NAME[name], _gold(), f"{name}/{TS.sub_tag(sub)}"
    logs, grads = _step(case, sub, "cpu", double=True)
    names = list(gold[f"{tag}/log_names"])
    assert sorted(logs) == names
    e_log = max(TS.scalar_err(v, logs[k]) for k, v in zip(names, gold[f"{tag}/log_values"]))
    fixture = TS.load_group(gold, f"{tag}/grad/")
    assert set(fixture) == set(grads)
    e_grad = max(TS.group_errs(fixture, grads, TS.ZERO_GRADIENTS[case.model]).values())
    assert e_log <= E_REF_MAX and e_grad <= E_REF_MAX, (tag, e_log, e_grad)
    return logs, grads, (e_log, e_grad)


def _within_rule(case, sub, logs, grads, what):
    """the device's logs and gradients against the float64 truth, within MARGIN x e_ref (logged values: or FLOOR); prints the ratios"""
    want_logs, want_grads, (e_log, e_grad) = _truth(case.name, sub)
    assert sorted(logs) == sorted(want_logs), (what, sorted(logs))
    assert set(grads) == set(want_grads), (what, sorted(set(grads) ^ set(want_grads)))
    d_log = max(TS.scalar_err(logs[k], want_logs[k]) for k in want_logs)
    d_grad = max(TS.group_errs(grads, want_grads, TS.ZERO_GRADIENTS[case.model]).values())
    print(f"{what}: logs {d_log:.2e} (e_ref {e_log:.2e}, ratio {d_log / e_log if e_log else float('inf'):.2f}) "
          f"gradients {d_grad:.2e} (e_ref {e_grad:.2e}, ratio {d_grad / e_grad if e_grad else float('inf'):.2f})")
    assert d_log <= max(MARGIN * e_log, FLOOR), (what, d_log, e_log)
    assert d_grad <= MARGIN * e_grad, (what, d_grad, e_grad)


@pytest.mark.parametrize("setting", SETTINGS, ids=_setting_id)
def test_step_on_the_device_against_the_references_step(setting):
    """Every case of the fixture in fp32 on the device.  shared_hash_dropout: the device draws its dropout masks from its
    own generator, so its numbers are another sample than the host-made fixture's -- there the logged names and the set of
    parameters with a gradient are compared, and test_rng_replay_on_the_device holds the replay."""
    case, sub = setting
    logs, grads = _step(case, sub, "cuda")
    tag = f"{case.name}/{TS.sub_tag(sub)}"
    assert sorted(logs) == list(_gold()[f"{tag}/log_names"])
    assert sorted(grads) == list(_gold()[f"{case.name}/trainable"])
    assert all(torch.isfinite(g).all() for g in grads.values()) and all(v == v for v in logs.values())
    if case.dropout == 0.0:
        _within_rule(case, sub, logs, grads, f"device {tag}")


@pytest.mark.parametrize("setting", FUSED_SETTINGS, ids=_setting_id)
def test_fused_losses_inside_the_step(setting, monkeypatch):
    """wv_rank_ap / wv_pair_loss reached through the step, single pass and gradient-cached (the loss sees the leaf emb_full,
    its kernel-made gradient is sliced and replayed through torch.autograd.backward(tensors, grad_tensors)): the library
    call happens exactly when `fused`, the parameter gradients of both paths agree within TOL and both keep the rule."""
    case, sub = setting
    calls = []
    for name in ("rank_ap", "pair_loss"):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _real=real, _name=name, **k: calls.append((_name, k.get("want_grad"))) or _real(*a, **k))
    want = [("pair_loss" if kind == "sch" else "rank_ap", True) for kind, _ in case.criteria if kind in TS.FUSED_KINDS]
    logs_f, grads_f = _step(case, sub, "cuda", fused=True)
    assert calls == want, calls
    calls.clear()
    logs_p, grads_p = _step(case, sub, "cuda", fused=False)
    assert calls == []
    tag = f"{case.name}/{TS.sub_tag(sub)}"
    d_log = max(TS.scalar_err(logs_f[k], logs_p[k]) for k in logs_p)
    d_grad = max(TS.group_errs(grads_f, grads_p, TS.ZERO_GRADIENTS[case.model]).values())
    print(f"{tag}: fused against plain: logs {d_log:.2e} gradients {d_grad:.2e}")
    assert sorted(logs_f) == sorted(logs_p) and d_log <= TS.TOL and d_grad <= TS.TOL
    _within_rule(case, sub, logs_f, grads_f, f"fused {tag}")
    _within_rule(case, sub, logs_p, grads_p, f"plain {tag}")


def test_rng_replay_on_the_device():
    """Dropout 0.5, 9 = 4 + 5 samples: the second forward of a micro-batch repeats the first one's masks, the masks of the
    other micro-batch's state would not, and after the step both streams stand where the first forwards left them."""
    case = TS.BY_NAME["shared_hash"]._replace(dropout=0.5)
    net = TS.wvhash_model(case, TS.load_state(_gold(), case)).cuda()
    criteria = [(c.cuda(), w) for c, w in TS.wvhash_criteria(case, _proxies(case))]
    x, y = TS.images(case).cuda(), TS.labels(case).cuda()
    seen = []
    hook = net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
    torch.manual_seed(77)
    backward_step(net, x, y, criteria, autocast_dtype=None, sub_batch=4)
    after = torch.rand(4, device="cuda"), torch.rand(4)
    in_step = list(seen)
    chunks = [(0, 4), (4, 9)]
    assert [tuple(t.shape) for t in in_step] == [(e - s, TS.NBITS) for s, e in chunks] * 2
    for i in range(2):
        err = TS.grad_err(in_step[2 + i], in_step[i])
        print(f"micro-batch {i}: replay against the first forward {err:.2e}")
        assert err <= TS.TOL
    # the first forwards alone, from the same seed
    seen.clear()
    torch.manual_seed(77)
    states = []
    with torch.no_grad():
        for s, e in chunks:
            states.append((torch.get_rng_state(), torch.cuda.get_rng_state()))
            net(x[s:e])
    alone = torch.rand(4, device="cuda"), torch.rand(4)
    first = list(seen)
    assert torch.equal(after[0], alone[0]) and torch.equal(after[1], alone[1])
    for i in range(2):
        assert TS.grad_err(first[i], in_step[i]) <= TS.TOL
    # each micro-batch under the OTHER one's state: other masks, other embeddings
    for i, (s, e) in enumerate(chunks):
        cpu_state, gpu_state = states[1 - i]
        torch.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(gpu_state)
        seen.clear()
        with torch.no_grad():
            net(x[s:e])
        err = TS.grad_err(seen[0], first[i])
        print(f"micro-batch {i} under the other state: {err:.2e}")
        assert err > 1000 * TS.TOL
    hook.remove()


@pytest.mark.parametrize("sub", TS.SUB_BATCHES, ids=TS.sub_tag)
def test_raw_batch_equals_its_expanded_input(sub):
    """A raw uint8 [8, 3, 28, 28] batch with a bound deferred SWTTransform against swt2d of it as 5-D input."""
    case = TS.BY_NAME["shared_hash"]
    x = torch.from_numpy(synth.natural_images(8, 28, 28, seed=5)).permute(0, 3, 1, 2).contiguous()
    assert x.dtype == torch.uint8
    y = synth.multi_hot_labels(8, TS.CLASSES, 0.2, 6)
    runs = []
    for raw in (True, False):
        net = TS.wvhash_model(case, TS.load_state(_gold(), case)).cuda()
        net.bind_transform(SWTTransform(level=1, wavelet="haar", defer=True))
        criteria = [(c.cuda(), w) for c, w in TS.wvhash_criteria(case, _proxies(case))]
        inp = x if raw else swt2d(x.cuda(), "haar", 1)
        assert inp.dim() == (4 if raw else 5)
        torch.manual_seed(5)
        logs = backward_step(net, inp, y, criteria, autocast_dtype=None, sub_batch=sub)
        runs.append((logs, {k: p.grad.detach().clone() for k, p in TS.trainable(net).items()}))
    (logs_raw, grads_raw), (logs_5d, grads_5d) = runs
    d_log = max(TS.scalar_err(logs_raw[k], logs_5d[k]) for k in logs_5d)
    d_grad = max(TS.group_errs(grads_raw, grads_5d, TS.ZERO_GRADIENTS[case.model]).values())
    print(f"raw against expanded, {TS.sub_tag(sub)}: logs {d_log:.2e} gradients {d_grad:.2e}")
    assert sorted(logs_raw) == sorted(logs_5d) and d_log <= TS.TOL and d_grad <= TS.TOL
