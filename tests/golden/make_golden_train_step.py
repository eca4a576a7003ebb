#!/usr/bin/env python3
"""Regenerates tests/golden/train_step_golden.npz.  Run in the BUILD container only (needs /root/reference), never on a
GPU machine:
    python tests/golden/make_golden_train_step.py

What it pins: wvhash.engine.train_step (backward_step, train_step, _criterion_loss, _micro_batches, the RNG replay), with
numbers the REFERENCE's own optimisation step produced here.

* `_capture_rng_state`, `_replay_rng_state`, `_split_into_microbatches`, `_single_pass_optimization`,
  `_gradient_cached_optimization`, `_batch_optimization` and `base_update` are cut out of
  /root/reference/main/engine/base_update.py with `ast` at generation time and compiled unmodified into a namespace
  (nothing of the source is stored).  `lib` there is a stand-in object whose create_label_matrix, DictAverage, LOGGER and
  get_gradient_norm are loaded from the reference by file path; `config` is a SimpleNamespace (experience.sub_batch,
  clip_grad, log_grad=False, warm_up=0, warm_up_key=None, step_per_epoch; memory=None); no scaler, no memory, no batch-mAP
  calculator.
* The functions call `.cuda()` on the batch: the batch tensors are instances of a torch.Tensor subclass whose cuda() returns
  self.  torch.cuda.is_available() is false here, so the reference's RNG capture is CPU-only.
* Models: the reference's own SharedDinoHashing (cross_attention_advanced; its last_ortho_loss is parameter-only) and
  DINOHashBaseline, imported by file path, on the seeded frozen stand-in backbone of tests/train_step_cases.py; every
  parameter and buffer filled by wvhash.synth.randomize_module under the case's seed.
* Losses: the reference's own HashLoss, SmoothAP / SupAP and SCHLoss, loaded as make_golden_train.py, make_golden_rank_ap.py
  and make_golden_pair_losses.py load them.

Per case of train_step_cases.CASES and sub_batch in (None, 4), from `_batch_optimization` on a freshly loaded model: the
logged names (sorted) and values (float64), the gradient of every trainable parameter (and of HashLoss's proxies), and
`rng_after` = torch.rand(4) of the global stream after the call.  For train_step_cases.STEP_CASES, from `base_update` on a
one-batch loader with an active clip_grad and AdamW on the net: every trainable parameter, HashLoss's proxies and the
BatchNorm running statistics after the step.  `split/sizes`: the chunk sizes of `_split_into_microbatches` for every
total <= 12 and sub_batch 2 ... 6.

Data only: tensors, key names, logged names.  One thread, fixed seeds: two runs give the same arrays.
"""
import ast
import contextlib
import importlib.util
import logging
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["TQDM_DISABLE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "image-retrieval-wavelet_amd"), HERE]

import train_step_cases as C  # noqa: E402
from make_golden import _cut, load_reference_heads  # noqa: E402
from make_golden_pair_losses import load_reference as load_reference_loss  # noqa: E402
from make_golden_rank_ap import load_reference as load_reference_rank_ap  # noqa: E402
from make_golden_single_band import load_reference_models  # noqa: E402
from make_golden_train import load_reference_hashloss  # noqa: E402
from wvhash import synth  # noqa: E402

REF = "/root/reference"
STEP_FUNCTIONS = ["_capture_rng_state", "_replay_rng_state", "_split_into_microbatches", "_single_pass_optimization",
                  "_gradient_cached_optimization", "_batch_optimization", "base_update"]


class HostBatch(torch.Tensor):
    """A batch tensor on a machine without a GPU: `.cuda()` is the tensor itself.  Slices and concatenations of a batch are
    batches (the step slices micro-batches and joins their labels before `.cuda()`); every other result is a plain tensor,
    so nothing of the subclass reaches the model's graph."""

    def cuda(self, *args, **kwargs):
        return self

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            ret = func(*args, **(kwargs or {}))
        return ret.as_subclass(cls) if func in (torch.Tensor.__getitem__, torch.cat) else ret


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference_step():
    """-> namespace holding the reference's step functions, compiled unmodified"""
    utils = types.ModuleType("refutils")
    utils.__path__ = [os.path.join(REF, "main", "utils")]
    sys.modules["refutils"] = utils
    for name in ("average_meter", "dict_average"):         # dict_average imports its sibling relatively
        spec = importlib.util.spec_from_file_location(f"refutils.{name}", os.path.join(REF, "main", "utils", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refutils.{name}"] = mod
        spec.loader.exec_module(mod)
    lib = types.SimpleNamespace(
        create_label_matrix=_load("ref_create_label_matrix", "main", "utils", "create_label_matrix.py").create_label_matrix,
        DictAverage=sys.modules["refutils.dict_average"].DictAverage,
        LOGGER=_load("ref_logger", "main", "utils", "logger.py").LOGGER,
        get_gradient_norm=_load("ref_get_gradient_norm", "main", "utils", "get_gradient_norm.py").get_gradient_norm)
    funcs = _cut(os.path.join(REF, "main", "engine", "base_update.py"), None, STEP_FUNCTIONS)
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "np": np, "os": os, "lib": lib, "contextmanager": contextlib.contextmanager,
          "tqdm": lambda loader, disable=None: loader, "compute_batch_map": None}
    exec(compile(mod, "<reference base_update.py (cut)>", "exec"), ns)
    return ns


def reference_classes():
    mda = load_reference_heads()
    mda.load_dinov2 = lambda *a, **k: C.Backbone()
    mda.print = lambda *a, **k: None
    base = load_reference_models()["DINOHashBaseline"]
    sys.modules["refmodels.dino_baseline"].load_dinov2 = lambda *a, **k: C.Backbone()
    rank = load_reference_rank_ap()
    models = {"shared": mda.SharedDinoHashing, "shared_plain": mda.SharedDinoHashing, "base": base}
    losses = {"HashLoss": load_reference_hashloss().HashLoss, "SmoothAP": rank.SmoothAP, "SupAP": rank.SupAP,
              "SCHLoss": load_reference_loss("dsch").SCHLoss}
    return models, losses


def config_of(sub_batch, clip_grad=None):
    return types.SimpleNamespace(memory=None, experience=types.SimpleNamespace(
        sub_batch=sub_batch, clip_grad=clip_grad, log_grad=False, warm_up=0, warm_up_key=None, step_per_epoch=10))


def batch_of(case):
    return {"image": C.images(case).as_subclass(HostBatch), "label": C.labels(case).as_subclass(HostBatch)}


def check_sch_masks(case):
    """SCHLoss: the fixture must lie where the reference's fp32 `S == 1` and the exact set relation give the same numbers
    (make_golden_pair_losses.py): alpha = 1, codes in [-1, 1] (tanh), n_bits >= D."""
    kw = C.LOSS_KWARGS["sch"]
    assert kw["alpha"] == 1 and kw["apply_tanh"] and kw["n_bits"] >= C.NBITS, case.name


def make():
    torch.set_num_threads(1)
    logging.getLogger("RETRIEVAL").setLevel(logging.ERROR)
    ns = load_reference_step()
    models, losses = reference_classes()
    out = {"cases": np.array([c.name for c in C.CASES])}

    sizes = np.zeros((len(C.SPLIT_TOTALS), len(C.SPLIT_SUBS), max(C.SPLIT_TOTALS)), dtype=np.int64)
    for i, total in enumerate(C.SPLIT_TOTALS):
        for j, sub in enumerate(C.SPLIT_SUBS):
            chunks = ns["_split_into_microbatches"]({"image": torch.zeros(total, 1), "label": torch.zeros(total)}, sub)
            got = [mb["image"].size(0) for mb in chunks]
            assert sum(got) == total
            sizes[i, j, :len(got)] = got
    out["split/sizes"] = sizes

    for case in C.CASES:
        if any(kind == "sch" for kind, _ in case.criteria):
            check_sch_masks(case)
        torch.manual_seed(case.seed)
        model = models[case.model](**C.model_kwargs(case))
        synth.randomize_module(model, 100 + case.seed)
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in state.items():
            out[f"{case.name}/state/{k}"] = v.numpy()
        out[f"{case.name}/trainable"] = np.array(sorted(C.trainable(model)))
        for sub in C.SUB_BATCHES:
            tag = f"{case.name}/{C.sub_tag(sub)}"
            model.load_state_dict(state, strict=True)
            model.train()
            model.zero_grad()
            criteria = C.criteria_of(case, losses)
            for crit, _ in criteria:
                if hasattr(crit, "proxies"):
                    out[f"{case.name}/proxies"] = crit.proxies.detach().clone().numpy()
            torch.manual_seed(4000 + case.seed)
            logs = ns["_batch_optimization"](config_of(sub), model, batch_of(case), criteria, None, None, 0, None)
            out[f"{tag}/rng_after"] = torch.rand(4).numpy()
            names = sorted(logs)
            out[f"{tag}/log_names"] = np.array(names)
            out[f"{tag}/log_values"] = np.array([logs[k] for k in names], dtype=np.float64)
            grads = {k: p.grad for k, p in C.trainable(model).items() if p.grad is not None}
            assert set(grads) == set(C.trainable(model)), (tag, sorted(set(C.trainable(model)) - set(grads)))
            top = max(float(g.abs().max()) for g in grads.values())
            for k, g in grads.items():
                assert torch.isfinite(g).all(), (tag, k)
                assert (float(g.abs().max()) <= 1e-6 * top) == (k in C.ZERO_GRADIENTS[case.model]), (tag, k)   # noise, nothing else
                out[f"{tag}/grad/{k}"] = g.detach().clone().numpy()
            for crit, _ in criteria:
                if hasattr(crit, "proxies"):
                    out[f"{tag}/grad_proxies"] = crit.proxies.grad.detach().clone().numpy()
            norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads.values()])))
            print(f"{tag}: logs {dict((k, round(v, 6)) for k, v in logs.items())} |grad| {norm:.4f} over {len(grads)} tensors")

            if (case.name, sub) not in C.STEP_CASES:
                continue
            assert norm > 4 * C.CLIP_GRAD, (tag, norm)              # the clip is active
            model.load_state_dict(state, strict=True)
            criteria = C.criteria_of(case, losses)
            opt = {"net": torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], **C.NET_OPT)}
            torch.manual_seed(4000 + case.seed)
            ns["base_update"](config_of(sub, C.CLIP_GRAD), model, [batch_of(case)], criteria, opt, {"on_step": []}, None, 0)
            for k, p in C.trainable(model).items():
                assert p.grad is None or not p.grad.any()           # zero_grad ran
                out[f"{tag}/after/{k}"] = p.detach().clone().numpy()
            for k, v in C.running_stats(model).items():
                out[f"{tag}/after_stats/{k}"] = v.detach().clone().numpy()
            for crit, _ in criteria:
                if hasattr(crit, "proxies"):
                    out[f"{tag}/after_proxies"] = crit.proxies.detach().clone().numpy()
    path = os.path.join(HERE, "train_step_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
    return out


if __name__ == "__main__":
    make()
