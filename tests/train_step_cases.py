"""Shared by tests/golden/make_golden_train_step.py, tests/test_train_step_golden.py and tests/test_gpu_train_step.py: the
cases of the training-step fixture (tests/golden/train_step_golden.npz), the seeded stand-in backbone, the seeded inputs
and the constructors of both sides' models and criteria.  No test functions.  Everything is made on the host from seeds.

The fixture holds what the REFERENCE's own `_batch_optimization` / `base_update` (main/engine/base_update.py:52-415)
produced on these cases: logged names and values, the gradient of every trainable parameter, the next draw of the global
RNG stream, and for STEP_CASES the parameters, HashLoss's proxies and the BatchNorm statistics after one optimizer step.

Sizes: embedding width 16, 4 heads, 4 queries, 16 bits, 12 classes, 8 x 8 images -- about 3 500 trainable values in the
Shared model, so that full gradients and states of every case fit a committed fixture.  Batches: 9 = 4 + 5 (the trailing
single sample merged into its predecessor), 8 = 4 + 4, 12 = 4 + 4 + 4.
"""
import collections

import torch
import torch.nn as nn

from pair_loss_cases import TOL, grad_err, scalar_err  # noqa: F401  (the project's figure and measures for fp32 twins)

EMBED = 16
NBITS = 16
CLASSES = 12
IMG = 8
SUB_BATCHES = (None, 4)
CLIP_GRAD = 0.01          # far below every case's gradient norm (asserted by the generator): the clip is active
NET_OPT = dict(lr=1e-2, eps=1e-3, weight_decay=1e-2)      # eps this large: AdamW's first step depends on the gradient's scale
LOSS_OPT = {"name": "AdamW", "kwargs": {"lr": 1e-2, "weight_decay": 1e-4}}

FUSION = {"type": "cross_attention_advanced", "output_dim": EMBED, "num_heads": 4, "num_queries": 4, "dropout": 0.0,
          "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}

Case = collections.namedtuple("Case", "name model dropout B labels criteria seed")
# criteria: [(kind, weight)]; kind names a constructor of `criteria_of`
CASES = [
    Case("shared_hash", "shared", 0.0, 9, "multi", [("hash", 1.0)], 11),
    Case("shared_hash_dropout", "shared", 0.1, 9, "multi", [("hash", 1.0)], 12),
    # the plain head's ortho loss is the Gram of the batch-mean attention weights: it differs between micro-batches, so a
    # weight other than the chunk's share of the batch (4/9, 5/9) shows, which a parameter-only ortho loss cannot tell
    Case("shared_plain_hash", "shared_plain", 0.0, 9, "multi", [("hash", 1.0)], 17),
    Case("shared_two", "shared", 0.0, 8, "multi", [("hash", 1.0), ("smooth", 0.5)], 13),
    Case("base_supap_multi", "base", 0.0, 12, "multi", [("sup", 1.0)], 14),
    Case("base_supap_ids", "base", 0.0, 12, "ids", [("sup", 1.0)], 15),
    Case("base_supap_ids_col", "base", 0.0, 12, "ids_col", [("sup", 1.0)], 15),
    Case("base_sch", "base", 0.0, 12, "multi", [("sch", 1.0)], 16),
]
BY_NAME = {c.name: c for c in CASES}
# (case, sub_batch) whose optimizer step is stored as well
STEP_CASES = [("shared_hash", None), ("shared_hash", 4), ("base_supap_ids_col", None)]
# _micro_batches against the reference's split: every total and sub_batch of this table
SPLIT_TOTALS = tuple(range(1, 13))
SPLIT_SUBS = tuple(range(2, 7))

LOSS_KWARGS = {
    "hash": dict(num_classes=CLASSES, embedding_size=NBITS, optimizer=LOSS_OPT),
    "smooth": dict(tau=0.01),
    "sup": dict(tau=0.01, rho=100, offset=1.44, delta=0.05),          # config/loss/roadmap.yaml
    "sch": dict(n_bits=NBITS, alpha=1, beta=1, apply_tanh=True),     # alpha = 1: the one setting where both `same` rules agree
}
LOSS_CLASS = {"hash": "HashLoss", "smooth": "SmoothAP", "sup": "SupAP", "sch": "SCHLoss"}
FUSED_KINDS = ("smooth", "sup", "sch")     # the criteria with a library path


# Gradients that are zero in exact arithmetic: norm2.bias adds the same vector to every row of the fused embedding, hash_fc
# (no bias) turns it into one constant per logit, and BatchNorm in train mode subtracts a batch's constant again.  What either
# side holds there is rounding noise (1e-8 beside gradients of 1e-1), which has no relative error: such a tensor is measured
# against the largest gradient element of the whole model instead of its own.
ZERO_GRADIENTS = {"shared": ("fusion_head.norm2.bias",), "shared_plain": ("fusion_head.norm2.bias",), "base": ()}


def group_errs(got, want, zero=()):
    """name -> grad_err of every tensor of `want`; the names in `zero` against the largest element of all of `want`"""
    top = max(float(w.abs().max()) for w in want.values())
    out = {}
    for k, w in want.items():
        if k in zero:
            out[k] = float((got[k].detach().double().cpu() - w.double().cpu()).abs().max()) / top
        else:
            out[k] = grad_err(got[k], w)
    return out


def sub_tag(sub):
    return "single" if sub is None else f"sub{sub}"


class Backbone(nn.Module):
    """[N, 3, H, W] -> {'x_norm_clstoken': [N, EMBED]}: 2 x 2 average pooling and one Linear, seeded."""

    def __init__(self, seed=0):
        super().__init__()
        self.embed_dim = EMBED
        self.pool = nn.AdaptiveAvgPool2d(2)
        self.proj = nn.Linear(12, EMBED)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(EMBED, 12, generator=g))
            self.proj.bias.copy_(0.1 * torch.randn(EMBED, generator=g))

    def forward(self, x):
        return {"x_norm_clstoken": self.proj(self.pool(x).flatten(1))}


def model_kwargs(case):
    """Constructor kwargs of the case's model, the same on both sides (wvhash adds backbone= / the reference's loader is
    replaced by Backbone)."""
    if case.model != "base":
        head = "cross_attention_advanced" if case.model == "shared" else "cross_attention_bottleneck"
        return dict(backbone_config={"name": "dinov2_vits14", "frozen": True},
                    fusion_config=dict(FUSION, type=head, dropout=case.dropout), binary_config={"nbits": NBITS})
    return dict(dino_backbone="dinov2_vits14", embed_dim=EMBED, binary_config={"nbits": NBITS}, frozen=True)


def images(case):
    """fp32 sub-bands [B, 3, 4, IMG, IMG] for the Shared model, a plain image batch [B, 3, IMG, IMG] for the baseline.
    shared_plain: the samples grow from 1/4 to 8 times unit scale, so the later micro-batch attends far more sharply than the
    first and the two see different ortho losses."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = (case.B, 3, 4, IMG, IMG) if case.model != "base" else (case.B, 3, IMG, IMG)
    x = torch.randn(*shape, generator=g)
    if case.model == "shared_plain":
        x = x * torch.logspace(-2, 3, case.B, base=2.0).view(-1, 1, 1, 1, 1)
    return x


def labels(case):
    """multi: fp32 multi-hot [B, 12], every row tagged; ids: int64 class ids [B] of 5 classes, id 0 present; ids_col: the
    same ids as [B, 1]"""
    from wvhash import synth
    if case.labels == "multi":
        return synth.multi_hot_labels(case.B, CLASSES, 0.2, 2000 + case.seed)
    g = torch.Generator().manual_seed(2000 + case.seed)
    ids = torch.randint(0, 5, (case.B,), generator=g)
    ids[0], ids[1] = 0, 3
    return ids.view(-1, 1) if case.labels == "ids_col" else ids


def wvhash_model(case, state=None):
    """wvhash's model of the case in train mode; state: a state dict to load strictly (the fixture's)"""
    from wvhash.models import DINOHashBaseline, SharedDinoHashing
    if case.model != "base":
        net = SharedDinoHashing(backbone=Backbone(), **model_kwargs(case))
    else:
        net = DINOHashBaseline(backbone=Backbone(), **model_kwargs(case))
    if state is not None:
        net.load_state_dict(state, strict=True)
    return net.train()


def criteria_of(case, classes, proxies=None):
    """[(module, weight)] from `classes` (name -> class: wvhash.losses or the reference's); HashLoss is constructed under
    the case's seed and then given `proxies` when the fixture's are at hand"""
    out = []
    for kind, weight in case.criteria:
        torch.manual_seed(3000 + case.seed)
        crit = classes[LOSS_CLASS[kind]](**LOSS_KWARGS[kind])
        if kind == "hash" and proxies is not None:
            with torch.no_grad():
                crit.proxies.copy_(proxies)
        out.append((crit, weight))
    return out


def wvhash_criteria(case, proxies=None):
    from wvhash import losses
    return criteria_of(case, {n: getattr(losses, n) for n in LOSS_CLASS.values()}, proxies)


def trainable(net):
    return {k: p for k, p in net.named_parameters() if p.requires_grad}


def running_stats(net):
    return {k: v for k, v in net.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}


def load_state(npz, case):
    prefix = f"{case.name}/state/"
    return {k[len(prefix):]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(prefix)}


def load_group(npz, prefix):
    return {k[len(prefix):]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(prefix)}
