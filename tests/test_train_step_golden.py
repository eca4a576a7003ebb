"""wvhash.engine.train_step against the REFERENCE's own optimisation step.
tests/golden/make_golden_train_step.py cuts `_batch_optimization`, `base_update` and what they call out of
/root/reference/main/engine/base_update.py:12-415, compiles them unmodified and runs them on the reference's own models
and losses in the build container; the fixture holds tensors, key names and logged names only.  Cases:
tests/train_step_cases.py.  CPU tests: the training path is stock PyTorch and follows its tensors' device, so the same
fp32 operations run on both sides and TOL (pair_loss_cases: 5e-5, what the project holds fp32 twins to against
reference-made goldens) has room to spare; the figures are printed.

What a case pins beyond "the same numbers": shared_hash -- the ortho loss is picked up, 9 samples split 4 + 5, `total_loss`
logged without ortho in the cached path and with it in the single pass; shared_plain_hash -- the ortho loss weighted by the
chunk's share of the batch (the plain head's ortho loss depends on the input, so 4/9, 5/9 and 1/2, 1/2 differ);
shared_hash_dropout -- the RNG snapshot and replay; shared_two -- weights and one log per class name; base_supap_* -- the
pairwise branch on a matrix target, on 1-D class ids and on the same ids as [B, 1]; base_sch -- the embedding branch."""
import os

import numpy as np
import pytest
import torch

import train_step_cases as C
from wvhash.engine import backward_step, train_step
from wvhash.engine.train_step import _micro_batches

SETTINGS = [(c, sub) for c in C.CASES for sub in C.SUB_BATCHES]


def _id(p):
    return f"{p[0].name}-{C.sub_tag(p[1])}"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "train_step_golden.npz"))


def _proxies(gold, case):
    key = f"{case.name}/proxies"
    return torch.from_numpy(gold[key]) if key in gold.files else None


def check_logs(logs, gold, tag, tol, what):
    """names equal the stored names; every value within tol (relative) -> the worst figure"""
    names = list(gold[f"{tag}/log_names"])
    assert sorted(logs) == names, (what, sorted(logs), names)
    errs = [C.scalar_err(logs[k], v) for k, v in zip(names, gold[f"{tag}/log_values"])]
    print(f"{what}: logs " + " ".join(f"{k} {e:.2e}" for k, e in zip(names, errs)))
    assert max(errs) <= tol, (what, dict(zip(names, errs)))
    return max(errs)


def check_group(got, want, tol, what, zero=()):
    """the same names; every tensor within tol by grad_err (train_step_cases.group_errs) -> the worst figure"""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    errs = C.group_errs(got, want, zero)
    worst = max(errs, key=errs.get)
    print(f"{what}: worst {errs[worst]:.2e} at {worst}")
    assert errs[worst] <= tol, (what, errs)
    return errs[worst]


@pytest.mark.parametrize("setting", SETTINGS, ids=_id)
def test_backward_step_is_the_references_batch_optimization(gold, setting):
    case, sub = setting
    tag = f"{case.name}/{C.sub_tag(sub)}"
    net = C.wvhash_model(case, C.load_state(gold, case))
    assert sorted(C.trainable(net)) == list(gold[f"{case.name}/trainable"])
    criteria = C.wvhash_criteria(case, _proxies(gold, case))
    torch.manual_seed(4000 + case.seed)
    logs = backward_step(net, C.images(case), C.labels(case), criteria, autocast_dtype=None, sub_batch=sub)
    rng_after = torch.rand(4).numpy()
    check_logs(logs, gold, tag, C.TOL, tag)
    grads = {k: p.grad for k, p in C.trainable(net).items() if p.grad is not None}
    check_group(grads, C.load_group(gold, f"{tag}/grad/"), C.TOL, f"{tag} gradients",
                C.ZERO_GRADIENTS[case.model])                               # and: the same set received one
    for crit, _ in criteria:
        if hasattr(crit, "proxies"):
            check_group({"proxies": crit.proxies.grad}, {"proxies": torch.from_numpy(gold[f"{tag}/grad_proxies"])}, C.TOL,
                        f"{tag} proxy gradient")
    assert np.array_equal(rng_after.view(np.int32), gold[f"{tag}/rng_after"].view(np.int32)), tag


@pytest.mark.parametrize("name,sub", C.STEP_CASES, ids=[f"{n}-{C.sub_tag(s)}" for n, s in C.STEP_CASES])
def test_train_step_is_the_references_base_update(gold, name, sub):
    """One batch through base_update with an active clip and AdamW on the net (eps large enough that the step depends on the
    gradient's scale: clipping after the step would show), HashLoss's own optimizer, BatchNorm statistics."""
    case = C.BY_NAME[name]
    tag = f"{name}/{C.sub_tag(sub)}"
    net = C.wvhash_model(case, C.load_state(gold, case))
    criteria = C.wvhash_criteria(case, _proxies(gold, case))
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], **C.NET_OPT)
    torch.manual_seed(4000 + case.seed)
    logs = train_step(net, C.images(case), C.labels(case), criteria, {"net": opt}, autocast_dtype=None, sub_batch=sub,
                      clip_grad=C.CLIP_GRAD)
    check_logs(logs, gold, tag, C.TOL, tag)
    before = C.load_state(gold, case)
    want = C.load_group(gold, f"{tag}/after/")
    moved = max(C.grad_err(want[k], before[k]) for k in want)
    print(f"{tag}: the step moved the parameters by {moved:.2e} of their largest value")
    check_group({k: p.detach() for k, p in C.trainable(net).items()}, want, C.TOL, f"{tag} parameters after the step")
    check_group(C.running_stats(net), C.load_group(gold, f"{tag}/after_stats/"), C.TOL, f"{tag} running statistics")
    for crit, _ in criteria:
        if hasattr(crit, "proxies"):
            check_group({"proxies": crit.proxies.detach()}, {"proxies": torch.from_numpy(gold[f"{tag}/after_proxies"])}, C.TOL,
                        f"{tag} proxies after their step")
            assert crit.proxies.grad is None or not crit.proxies.grad.any()
    assert all(p.grad is None or not p.grad.any() for p in net.parameters())


def test_micro_batches_are_the_references_split(gold):
    sizes = gold["split/sizes"]
    for i, total in enumerate(C.SPLIT_TOTALS):
        for j, sub in enumerate(C.SPLIT_SUBS):
            chunks = _micro_batches(total, sub)
            want = [int(n) for n in sizes[i, j] if n]
            assert [e - s for s, e in chunks] == want, (total, sub, chunks, want)
            assert chunks[0][0] == 0 and chunks[-1][1] == total and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
