"""The proxy hashing loss the reference's headline runs train with, so that the training step of configs c2 / c4
 can be exercised: same name, kwargs, parameters and numbers as
/root/reference/main/losses/hash_loss.py:17-59 (class-proxy BCE on scaled cosine similarities of tanh'ed logits +
quantisation pull towards +-1; the proxies have their own optimizer, stepped by the training loop).
Plain PyTorch: training is outside the accelerated path.

And the two pairwise hashing baselines, SCHLoss (main/losses/dsch.py:6-59, `loss: dsch`) and HashNetAdapter / HashNetLoss
(main/losses/hashnet_loss.py:9-66): the same names, kwargs, attributes and numbers, each with two paths that agree to fp32
rounding -- stock PyTorch ops under autograd (CPU tensors, fp64, large or non-0/1 label shapes), and one library call for
the loss and its gradient w.r.t. the embeddings (wv_pair_loss, csrc/pair_loss.hip) behind a torch.autograd.Function for CUDA
tensors.  `module.fused = False` forces the plain path; neither path ever moves a tensor to another device."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .engine._args import anchor, gate


class HashLoss(nn.Module):
    takes_embeddings = True

    def __init__(self, num_classes=20, embedding_size=64, quant_weight=0.1, scale=15.0, **kwargs):
        super().__init__()
        self.quant_weight, self.scale = quant_weight, scale
        # randn first, like the reference (:25-26): the values are overwritten, but the global RNG stream must be consumed the
        # same way or everything seeded after the loss differs from a reference run with the same seed
        self.proxies = nn.Parameter(torch.randn(num_classes, embedding_size))
        nn.init.xavier_uniform_(self.proxies)
        cfg = kwargs.get("optimizer") or {"name": "AdamW", "kwargs": {"lr": 1e-4, "weight_decay": 1e-4}}
        name = cfg.get("name", "AdamW") if isinstance(cfg, dict) else getattr(cfg, "name", "AdamW")
        kw = (cfg.get("kwargs", {}) if isinstance(cfg, dict) else getattr(cfg, "kwargs", {})) or {}
        self.loss_optimizer = getattr(torch.optim, name)(self.parameters(), **dict(kw))

    def forward(self, embeddings, labels, **kwargs):
        codes = torch.tanh(embeddings)
        sims = F.normalize(codes, p=2, dim=1) @ F.normalize(self.proxies, p=2, dim=1).t()
        bce = F.binary_cross_entropy_with_logits(sims * self.scale, labels.float())
        quant = (codes.abs() - 1.0).abs().mean()
        return bce + self.quant_weight * quant

    def step(self):
        self.loss_optimizer.step()
        self.loss_optimizer.zero_grad()

    # the proxies' optimizer travels inside the loss's state_dict (hash_loss.py:50-59): a reference-made checkpoint's
    # loss state loads strictly, and the moments survive a resume
    def state_dict(self, destination=None, prefix="", keep_vars=False):
        sd = super().state_dict(destination=destination, prefix=prefix, keep_vars=keep_vars)
        sd["optimizer_state"] = self.loss_optimizer.state_dict()
        return sd

    def load_state_dict(self, state_dict, strict=True):
        state_dict = dict(state_dict)
        optimizer_state = state_dict.pop("optimizer_state", None)
        out = super().load_state_dict(state_dict, strict)
        if optimizer_state is not None:
            self.loss_optimizer.load_state_dict(optimizer_state)
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Pairwise hashing losses
# ---------------------------------------------------------------------------------------------------------------------
PAIR_LOSS_ROWS_MAX = _lib.WV_PAIR_LOSS_ROWS_MAX      # rows of a batch wv_pair_loss takes
PAIR_LOSS_D_MAX = 512                                # ... and its widest embedding
PAIR_LOSS_CLASSES_MAX = 128                          # two packed label words
_HALF = (torch.bfloat16, torch.float16)


def pair_loss_params(kind, apply_tanh=False, pre_scale=1.0, nbits=64.0, alpha=0.1, beta=0.1):
    """wv_pair_loss_params of include/wvhash.h.  kind: 'sch' or 'hashnet' (or the WV_PAIR_LOSS_* value)."""
    kind = {"sch": _lib.WV_PAIR_LOSS_SCH, "hashnet": _lib.WV_PAIR_LOSS_HASHNET}.get(kind, kind)
    return _lib.PairLossParams(int(kind), int(bool(apply_tanh)), float(pre_scale), float(nbits), float(alpha), float(beta))


def _pair_loss(what, e, labels_packed, params, want_grad, device_type):
    """The arguments of pair_loss on either side, gated (engine/_args.py), and the call -> (out float32 [3], grad or None)"""
    dev = anchor(e, what, "e", device_type)
    if e.dtype in _HALF:
        e = e.float()                                # exact
    e = gate(e, what, "e", torch.float32, dev, (None, None))
    labels_packed = gate(labels_packed, what, "labels_packed", torch.int64, dev, (e.shape[0], None))
    if not isinstance(params, _lib.PairLossParams):
        raise ValueError(f"{what}: params: expected a PairLossParams (pair_loss_params()), got {type(params).__name__}")
    B, D = e.shape
    lw = labels_packed.shape[1]
    out = torch.empty(3, dtype=torch.float32, device=dev)
    grad = torch.empty_like(e) if want_grad else None
    if device_type == "cpu":
        rc = _lib.load().wv_pair_loss_cpu(_lib.ptr(e), _lib.ptr(labels_packed), lw, B, D, ctypes.byref(params), _lib.ptr(out),
                                          _lib.ptr(grad))
        name = "wv_pair_loss_cpu"
    else:
        lib = _lib.require_gpu()
        with torch.cuda.device(dev):
            nbytes = lib.wv_pair_loss_workspace_bytes(B, D)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            rc = lib.wv_pair_loss(_lib.ptr(e), _lib.ptr(labels_packed), lw, B, D, ctypes.byref(params), _lib.ptr(out),
                                  _lib.ptr(grad), _lib.ptr(ws), ctypes.c_size_t(nbytes), _lib.stream_ptr())
        name = "wv_pair_loss"
    if rc == _lib.WV_ENOTSUP:
        raise _lib.WvhashUnsupported(f"{name}: " + _lib.load().wv_last_error().decode(errors="replace"))
    _lib.check(rc, name)
    return out, grad


def pair_loss(e, labels_packed, params, want_grad=True):
    """SCHLoss / HashNetLoss with its gradient in one library call (wv_pair_loss, two launches on the current stream).
    e [B, D] on a CUDA device, fp32 (bf16 / fp16 are widened); labels_packed int64 [B, 1 or 2] (pack_labels); params:
    pair_loss_params() -> (out float32 [3]: loss, part 1, part 2;  grad float32 [B, D] = d loss / d e, or None when not
    wanted: the kernel then skips that part).  WvhashUnsupported above PAIR_LOSS_ROWS_MAX rows or D > 512."""
    return _pair_loss("pair_loss", e, labels_packed, params, want_grad, "cuda")


def pair_loss_host(e, labels_packed, params, want_grad=True):
    """pair_loss on host tensors, over the host twin wv_pair_loss_cpu: the same rules and per-pair code, fp32."""
    return _pair_loss("pair_loss_host", e, labels_packed, params, want_grad, "cpu")


class _FusedPairLoss(torch.autograd.Function):
    """loss = wv_pair_loss(e); the gradient the same call returned is kept for backward."""

    @staticmethod
    def forward(ctx, emb, labels_packed, params, want):
        # want: grad mode was on at the call and emb requires grad; otherwise the gradient pointer is null
        out, grad = pair_loss(emb.detach(), labels_packed, params, want_grad=want)
        if want:
            ctx.save_for_backward(grad)
        ctx.in_dtype = emb.dtype
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad_output * grad).to(ctx.in_dtype), None, None, None


class _PairLossPaths:
    """What SCHLoss and HashNetLoss share: the label rule, the choice between the two paths, the widening."""
    fused = True            # False: always the plain path
    check_labels = True     # False: labels are promised to be 0/1 -- skips one reduction and a sync per call

    @staticmethod
    def _labels_2d(what, labels):
        if labels.dim() != 2:
            raise ValueError(f"{what}: labels must be 2-D multi-hot [B, classes], got shape {tuple(labels.shape)} "
                             "(class-id labels have no pairwise relation here)")

    def _takes_fused(self, emb, labels):
        if not (self.fused and emb.is_cuda and emb.dim() == 2 and emb.dtype in (torch.float32,) + _HALF):
            return False
        if emb.shape[0] > PAIR_LOSS_ROWS_MAX or emb.shape[1] > PAIR_LOSS_D_MAX or emb.shape[0] < 1 or emb.shape[1] < 1:
            return False
        if not 1 <= labels.shape[1] <= PAIR_LOSS_CLASSES_MAX:
            return False
        return not self.check_labels or bool(((labels == 0) | (labels == 1)).all())

    def _fused(self, emb, labels, params):
        from .engine.hamming import pack_labels
        want = torch.is_grad_enabled() and emb.requires_grad      # the Function itself runs with grad mode off
        return _FusedPairLoss.apply(emb, pack_labels(labels.to(emb.device), check=False), params, want)

    @staticmethod
    def _widened(emb, labels):
        """Operands of the plain path: bf16 / fp16 widened, labels in the embeddings' dtype, on the embeddings' device"""
        emb = emb.float() if emb.dtype in _HALF else emb
        return emb, labels.to(device=emb.device, dtype=emb.dtype)


class SCHLoss(nn.Module, _PairLossPaths):
    """DSCH loss (main/losses/dsch.py).  `batch` must hold codes in [-1, 1]: models that emit raw logits set apply_tanh.
    Labels: 2-D multi-hot.  With L the label matrix, n_i = |L_i|, c_ij = |L_i & L_j|, G = u u^T, k = n_bits:
      S = c / sqrt(n_i n_j) (0 where n_i n_j = 0);  same: c = n_i = n_j > 0;  disjoint: c = 0
      lambda = (1 - S) k / 2;  lambda_l = max(lambda - 3, 0), k / 2 where disjoint
      W_l = 0 | beta | 1,  W_u = alpha | 0 | 1  for same | disjoint | other;  H = (k - G) / 2
      loss = |relu(lambda_l - H) W_l|_F / B^2 + |relu(H - lambda) W_u|_F / B^2
    `same` is the exact set relation; the reference tests S == 1 on an fp32 product of normalised rows, which holds for
    some label counts and not for others.  With alpha = 1 (config/loss/dsch.yaml) both give the same numbers."""
    takes_embeddings = True

    def __init__(self, n_bits=64, alpha=0.1, beta=0.1, apply_tanh=False, *args, **kwargs):
        super().__init__()
        self.n_bits = n_bits
        self.alpha = alpha
        self.beta = beta
        self.apply_tanh = apply_tanh
        self.max_func = torch.nn.ReLU()

    def forward(self, batch, labels):
        self._labels_2d("SCHLoss", labels)
        if self._takes_fused(batch, labels):
            return self._fused(batch, labels, pair_loss_params("sch", self.apply_tanh, 1.0, self.n_bits, self.alpha, self.beta))
        with torch.autocast(batch.device.type, enabled=False):
            return self.plain(*self._widened(batch, labels))

    def plain(self, batch, labels):
        """Stock PyTorch ops, differentiable by autograd, in the dtype of `batch`."""
        if self.apply_tanh:
            batch = torch.tanh(batch)
        B, k = labels.size(0), self.n_bits
        c = labels @ labels.t()
        n = (labels * labels).sum(1)
        nn_ = n[:, None] * n[None, :]
        S = torch.where(nn_ > 0, c / nn_.clamp(min=1e-30).sqrt(), torch.zeros_like(c))
        same = (c == n[:, None]) & (c == n[None, :]) & (c > 0)
        disjoint = c == 0
        S = torch.where(same, torch.ones_like(S), S)
        lam = (1 - S) * k / 2
        lam_l = torch.where(disjoint, torch.full_like(lam, k / 2), (lam - 3).clamp(min=0))
        one = torch.ones_like(lam)
        W_l = torch.where(same, 0 * one, torch.where(disjoint, self.beta * one, one))
        W_u = torch.where(same, self.alpha * one, torch.where(disjoint, 0 * one, one))
        H = (k - batch @ batch.t()) / 2
        loss1 = torch.norm(self.max_func(lam_l - H) * W_l) / (B * B)
        loss2 = torch.norm(self.max_func(H - lam) * W_u) / (B * B)
        return loss1 + loss2


class HashNetLoss(nn.Module, _PairLossPaths):
    """HashNet (ICCV 2017) pairwise loss, main/losses/hashnet_loss.py:44-66:  u = tanh(scale e), P = [c > 0],
    dp = alpha G, t = softplus(dp) - P dp, loss = sum_P t / S1 + sum_notP t / S0 (the reference's masked rescaling reduces to
    this; an empty class contributes nothing)."""

    def __init__(self, config, bit):
        super().__init__()
        self.scale = 1

    def forward(self, u, y, ind, config):
        self._labels_2d("HashNetLoss", y)
        alpha = config["alpha"]
        if self._takes_fused(u, y):
            return self._fused(u, y, pair_loss_params("hashnet", True, self.scale, 0.0, alpha, 0.0))
        with torch.autocast(u.device.type, enabled=False):
            return self.plain(*self._widened(u, y), alpha)

    def plain(self, u, y, alpha):
        u = torch.tanh(self.scale * u)
        P = ((y @ y.t()) > 0).to(u.dtype)
        dp = alpha * (u @ u.t())
        x = (1 - 2 * P) * dp
        t = torch.logaddexp(x, torch.zeros_like(x))           # softplus(dp) - P dp without the difference of large numbers
        S1 = P.sum()
        S0 = P.numel() - S1
        return (t * P).sum() / S1.clamp(min=1) + (t * (1 - P)).sum() / S0.clamp(min=1)


class HashNetAdapter(nn.Module):
    """HashNetLoss behind the training loop's loss interface (main/losses/hashnet_loss.py:9-36): step() counts batches and
    raises the continuation scale by one every `step_continuation` epochs of `batches_per_epoch` batches.
    Two behaviours of the reference are kept: forward passes alpha = 0.1 whatever the constructor got, and the step
    counter is not part of the state_dict, so the scale restarts at 1 on resume."""
    takes_embeddings = True

    def __init__(self, embedding_size=64, alpha=0.1, step_continuation=20, batches_per_epoch=49, **kwargs):
        super().__init__()
        config = {"alpha": alpha, "step_continuation": step_continuation}
        self.criterion = HashNetLoss(config=config, bit=embedding_size)
        self.step_continuation = step_continuation
        self.batches_per_epoch = batches_per_epoch
        self.global_batch_step = 0

    # the path switches live on the criterion, which chooses the path
    fused = property(lambda self: self.criterion.fused, lambda self, v: setattr(self.criterion, "fused", v))
    check_labels = property(lambda self: self.criterion.check_labels, lambda self, v: setattr(self.criterion, "check_labels", v))

    def forward(self, embeddings, labels, **kwargs):
        return self.criterion(u=embeddings, y=labels, ind=None, config={"alpha": 0.1})

    def step(self):
        self.global_batch_step += 1
        current_real_epoch = self.global_batch_step // self.batches_per_epoch
        self.criterion.scale = (current_real_epoch // self.step_continuation) + 1
