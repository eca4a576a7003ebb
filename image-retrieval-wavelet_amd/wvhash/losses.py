"""The proxy hashing loss the reference's headline runs train with, so that the training step of configs c2 / c4
 can be exercised: same name, kwargs, parameters and numbers as
/root/reference/main/losses/hash_loss.py:17-59 (class-proxy BCE on scaled cosine similarities of tanh'ed logits +
quantisation pull towards +-1; the proxies have their own optimizer, stepped by the training loop).
Plain PyTorch: training is outside the accelerated path.

And the two pairwise hashing baselines, SCHLoss (main/losses/dsch.py:6-59, `loss: dsch`) and HashNetAdapter / HashNetLoss
(main/losses/hashnet_loss.py:9-66): the same names, kwargs, attributes and numbers, each with two paths that agree to fp32
rounding -- stock PyTorch ops under autograd (CPU tensors, fp64, large or non-0/1 label shapes), and one library call for
the loss and its gradient w.r.t. the embeddings (wv_pair_loss, csrc/pair_loss.hip) behind a torch.autograd.Function for CUDA
tensors.  `module.fused = False` forces the plain path; neither path ever moves a tensor to another device.

And the rank-approximation AP losses on score matrices, SmoothRankAP / SmoothAP / SupAP / HeavisideAP
(main/losses/smooth_rank_ap.py; SupAP is the ranking part of `loss: roadmap`), with the same two paths: the fused one is
wv_rank_ap (csrc/rank_ap.hip), AP per query row and its gradient with no [B, B, B] tensor."""
import collections
import ctypes
import math
from functools import partial

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
# Fused losses: the library call, the autograd Function and the path switch that every one of them uses
# ---------------------------------------------------------------------------------------------------------------------
_HALF = (torch.bfloat16, torch.float16)

# What differs between the library calls of two fused losses.  Entry points have the shape
#   stem(x, second, *dims, params, out, grad, workspace, workspace_bytes, stream), stem_cpu without the last three
#   stem          the entry point; stem_cpu is its host twin, stem_workspace_bytes sizes its workspace
#   params_type   the params struct, params_fn the name of the function that builds one (for the error message)
#   first         argument name of the input x, fp32 [B, *]
#   second        name, dtype and shape (a function of x) of the second tensor
#   out_len       x -> length of the fp32 output
#   dims          (x, second) -> the int arguments between the tensors and the params
#   ws_args       (x, params) -> the arguments of stem_workspace_bytes
_FusedOp = collections.namedtuple("_FusedOp", "stem params_type params_fn first second out_len dims ws_args")

_PAIR_LOSS = _FusedOp("wv_pair_loss", _lib.PairLossParams, "pair_loss_params", "e",
                      ("labels_packed", torch.int64, lambda e: (e.shape[0], None)), lambda e: 3,
                      lambda e, lp: (lp.shape[1],) + tuple(e.shape), lambda e, params: tuple(e.shape))
_RANK_AP = _FusedOp("wv_rank_ap", _lib.RankApParams, "rank_ap_params", "scores",
                    ("target", torch.float32, lambda s: tuple(s.shape)), lambda s: s.shape[0],
                    lambda s, t: tuple(s.shape), lambda s, params: tuple(s.shape) + (params.form,))


def _fused_call(op, what, x, second, params, want_grad, device_type):
    """The arguments of a fused loss on either side, gated (engine/_args.py), and the call -> (out float32, grad or None)"""
    dev = anchor(x, what, op.first, device_type)
    if x.dtype in _HALF:
        x = x.float()                                # exact
    x = gate(x, what, op.first, torch.float32, dev, (None, None))
    second_name, second_dtype, second_shape = op.second
    second = gate(second, what, second_name, second_dtype, dev, second_shape(x))
    if not isinstance(params, op.params_type):
        raise ValueError(f"{what}: params: expected a {op.params_type.__name__} ({op.params_fn}()), "
                         f"got {type(params).__name__}")
    out = torch.empty(op.out_len(x), dtype=torch.float32, device=dev)
    grad = torch.empty_like(x) if want_grad else None
    args = (_lib.ptr(x), _lib.ptr(second), *op.dims(x, second), ctypes.byref(params), _lib.ptr(out), _lib.ptr(grad))
    if device_type == "cpu":
        name = op.stem + "_cpu"
        rc = getattr(_lib.load(), name)(*args)
    else:
        name = op.stem
        lib = _lib.require_gpu()
        with torch.cuda.device(dev):
            nbytes = getattr(lib, name + "_workspace_bytes")(*op.ws_args(x, params))
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            rc = getattr(lib, name)(*args, _lib.ptr(ws), ctypes.c_size_t(nbytes), _lib.stream_ptr())
    _lib.check(rc, name, unsupported=True)
    return out, grad


class _FusedLoss(torch.autograd.Function):
    """value = call(x): pair_loss, rank_ap or a host twin; the gradient the same call returned is kept for backward.
    pick: the element of the call's output that is the value (0: the loss of pair_loss), None: all of it (the ap of
    rank_ap, whose gradient row q belongs to ap[q])."""

    @staticmethod
    def forward(ctx, call, pick, x, second, params, want):
        # want: grad mode was on at the call and x requires grad; otherwise the gradient pointer is null
        out, grad = call(x.detach(), second, params, want_grad=want)
        if want:
            ctx.save_for_backward(grad)
        ctx.in_dtype = x.dtype
        return out if pick is None else out[pick]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        # grad_output over the gradient's trailing dimensions: a [B] one scales [B, M] row by row; a 0-dim one scales [B, D]
        # as it is (reshaped to [1, 1] it gives the same bits for 5 us more host time per backward)
        if grad_output.dim():
            grad_output = grad_output.reshape(grad_output.shape + (1,) * (grad.dim() - grad_output.dim()))
        return None, None, (grad_output * grad).to(ctx.in_dtype), None, None, None


class _FusedPaths:
    """What SCHLoss, HashNetLoss and SmoothRankAP share: the two switches, what any fused path asks of its input, the way
    into the Function, the operands of the plain path.  A family adds its shape limits, its label rule and its params."""
    fused = True            # False: always the plain path
    check_labels = True     # False: labels are promised to be what the fused path takes -- skips one reduction and a sync per call

    def _fusable(self, x):
        return self.fused and x.is_cuda and x.dtype in (torch.float32,) + _HALF

    @staticmethod
    def _fused(call, pick, x, second, params):
        """call: the public wrapper, looked up in this module when the family calls (tests count its calls)"""
        want = torch.is_grad_enabled() and x.requires_grad      # the Function itself runs with grad mode off
        return _FusedLoss.apply(call, pick, x, second, params, want)

    @staticmethod
    def _run_plain(fn, x, labels, *args):
        """fn(x, labels, *args) out of autocast's reach: bf16 / fp16 x widened, labels in x's dtype, on x's device"""
        with torch.autocast(x.device.type, enabled=False):
            wide = x.float() if x.dtype in _HALF else x
            return fn(wide, labels.to(device=wide.device, dtype=wide.dtype), *args)


# ---------------------------------------------------------------------------------------------------------------------
# Pairwise hashing losses
# ---------------------------------------------------------------------------------------------------------------------
PAIR_LOSS_ROWS_MAX = _lib.WV_PAIR_LOSS_ROWS_MAX      # rows of a batch wv_pair_loss takes
PAIR_LOSS_D_MAX = 512                                # ... and its widest embedding
PAIR_LOSS_CLASSES_MAX = 128                          # two packed label words


def pair_loss_params(kind, apply_tanh=False, pre_scale=1.0, nbits=64.0, alpha=0.1, beta=0.1):
    """wv_pair_loss_params of include/wvhash.h.  kind: 'sch' or 'hashnet' (or the WV_PAIR_LOSS_* value)."""
    kind = {"sch": _lib.WV_PAIR_LOSS_SCH, "hashnet": _lib.WV_PAIR_LOSS_HASHNET}.get(kind, kind)
    return _lib.PairLossParams(int(kind), int(bool(apply_tanh)), float(pre_scale), float(nbits), float(alpha), float(beta))


def pair_loss(e, labels_packed, params, want_grad=True):
    """SCHLoss / HashNetLoss with its gradient in one library call (wv_pair_loss, two launches on the current stream).
    e [B, D] on a CUDA device, fp32 (bf16 / fp16 are widened); labels_packed int64 [B, 1 or 2] (pack_labels); params:
    pair_loss_params() -> (out float32 [3]: loss, part 1, part 2;  grad float32 [B, D] = d loss / d e, or None when not
    wanted: the kernel then skips that part).  WvhashUnsupported above PAIR_LOSS_ROWS_MAX rows or D > 512."""
    return _fused_call(_PAIR_LOSS, "pair_loss", e, labels_packed, params, want_grad, "cuda")


def pair_loss_host(e, labels_packed, params, want_grad=True):
    """pair_loss on host tensors, over the host twin wv_pair_loss_cpu: the same rules and per-pair code, fp32."""
    return _fused_call(_PAIR_LOSS, "pair_loss_host", e, labels_packed, params, want_grad, "cpu")


class _PairLossPaths(_FusedPaths):
    """The pairwise family's own: 2-D multi-hot 0/1 labels, packed; the limits of wv_pair_loss."""

    @staticmethod
    def _labels_2d(what, labels):
        if labels.dim() != 2:
            raise ValueError(f"{what}: labels must be 2-D multi-hot [B, classes], got shape {tuple(labels.shape)} "
                             "(class-id labels have no pairwise relation here)")

    def _takes_fused(self, emb, labels):
        if not (self._fusable(emb) and emb.dim() == 2):
            return False
        if emb.shape[0] > PAIR_LOSS_ROWS_MAX or emb.shape[1] > PAIR_LOSS_D_MAX or emb.shape[0] < 1 or emb.shape[1] < 1:
            return False
        if not 1 <= labels.shape[1] <= PAIR_LOSS_CLASSES_MAX:
            return False
        return not self.check_labels or bool(((labels == 0) | (labels == 1)).all())

    def _fused_pair(self, emb, labels, params):
        from .engine.hamming import pack_labels
        return self._fused(pair_loss, 0, emb, pack_labels(labels.to(emb.device), check=False), params)


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
            return self._fused_pair(batch, labels, pair_loss_params("sch", self.apply_tanh, 1.0, self.n_bits, self.alpha, self.beta))
        return self._run_plain(self.plain, batch, labels)

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
            return self._fused_pair(u, y, pair_loss_params("hashnet", True, self.scale, 0.0, alpha, 0.0))
        return self._run_plain(self.plain, u, y, alpha)

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


# ---------------------------------------------------------------------------------------------------------------------
# Rank-approximation AP losses
# ---------------------------------------------------------------------------------------------------------------------
RANK_AP_COLS_MAX = _lib.WV_RANK_AP_COLS_MAX          # rows and columns of a score matrix wv_rank_ap takes


def rank_ap_params(kind, form, tau=0.01, rho=100.0, offset=0.0, delta=0.0, start=0.5):
    """wv_rank_ap_params of include/wvhash.h.  kind: 'smooth' or 'sup', form: 'quick' or 'general' (or the WV_RANK_AP_*
    values); offset is a number: resolve the reference's offset=None with sup_offset()."""
    kind = {"smooth": _lib.WV_RANK_AP_SMOOTH, "sup": _lib.WV_RANK_AP_SUP}.get(kind, kind)
    form = {"quick": _lib.WV_RANK_AP_QUICK, "general": _lib.WV_RANK_AP_GENERAL}.get(form, form)
    return _lib.RankApParams(int(kind), int(form), float(tau), float(rho), float(offset), float(delta), float(start))


def sup_offset(tau, delta, start):
    """What step_rank makes of offset=None: start + sigmoid_tau(delta)"""
    return start + 1.0 / (1.0 + math.exp(min(max(-delta / tau, -50.0), 50.0)))


def rank_ap(scores, target, params, want_grad=True):
    """SmoothAP / SupAP of every query row with its gradient in one library call (wv_rank_ap, two or three launches on the
    current stream).  scores [B, M] on a CUDA device, fp32 (bf16 / fp16 are widened); target float32 [B, M] of 0 / 1; params:
    rank_ap_params() -> (ap float32 [B];  grad float32 [B, M] = d ap[q] / d scores[q, :], or None when not wanted: the kernel
    then skips that part).  A row without a positive: ap 0, grad 0.  WvhashUnsupported above RANK_AP_COLS_MAX rows or columns."""
    return _fused_call(_RANK_AP, "rank_ap", scores, target, params, want_grad, "cuda")


def rank_ap_host(scores, target, params, want_grad=True):
    """rank_ap on host tensors, over the host twin wv_rank_ap_cpu: the same rules and per-pair code."""
    return _fused_call(_RANK_AP, "rank_ap_host", scores, target, params, want_grad, "cpu")


class _Heaviside(torch.autograd.Function):
    """torch.heaviside with no gradient (smooth_rank_ap.py:13-19)"""

    @staticmethod
    def forward(ctx, inputs, val):
        return torch.heaviside(inputs, torch.as_tensor(val, device=inputs.device, dtype=inputs.dtype))

    @staticmethod
    def backward(ctx, grad_output):
        return None, None


def heaviside(tens, val=1., target=None, general=None):
    return _Heaviside.apply(tens, val)


def tau_sigmoid(tensor, tau, target=None, general=None):
    """temperature controlled sigmoid, the exponent clamped to [-50, 50] (smooth_rank_ap.py:25-33)"""
    return 1.0 / (1. + (-tensor / tau).clamp(-50, 50).exp())


def step_rank(tens, tau, rho, offset=None, delta=None, start=0.5, target=None, general=False):
    """SupAP's rank approximation (smooth_rank_ap.py:36-64) as one expression instead of masked assignments in place: the
    same regions, the same values, differentiable by autograd.  tens [..., i, j] = S[q, j] - S[q, i].
    general: target is the query's positive mask [M]; otherwise the whole target [B, B], and a pair (q, i, j) is a target
    pair where rows i and j of it share a column and T[q, j] is set.
    tau as 'n_p' (two temperatures, negative and positive side): the pieces are read as numbers."""
    if general:
        tgt = target.bool().view(1, -1).expand(tens.size(0), -1)
    else:
        t = target.float()
        tgt = ((t @ t.t()) > 0) & target.bool().unsqueeze(1)
    tau_n, tau_p = (float(x) for x in tau.split("_")) if isinstance(tau, str) else (tau, tau)
    if delta is None:
        up = rho * tens + offset
    else:
        if offset is None:
            offset = sup_offset(tau_p, delta, start)
        up = torch.where(tens > delta, rho * (tens - delta) + offset, start + tau_sigmoid(tens, tau_p))
    return torch.where(tgt, heaviside(tens), torch.where(tens > 0, up, tau_sigmoid(tens, tau_n)))


class SmoothRankAP(nn.Module, _FusedPaths):
    """AP of every query row under a smooth rank (main/losses/smooth_rank_ap.py:67-161): same names, kwargs, asserts, choice
    between the two forms and return types.  scores, target [B, M]; no `takes_embeddings`: train_step hands over the score
    matrix emb @ emb.t() and the label matrix.

    quick form (square input):  [B, B, B] tensors, a pair (q, i, j) weighted by T[i, j]
    general form (B != M or force_general): a loop over the queries, weighted by T[q, j]
    The two are different functions on multi-hot label matrices, as in the reference.

    Two paths.  plain: stock PyTorch ops under autograd, on any device, in the dtype of `scores` (bf16 / fp16 widened to
    fp32) -- fp64, CPU tensors, targets that are not 0 / 1, a row without a positive (the reference's NaN), a quick-form
    target with a zero on its diagonal, a `tau` string, anything above RANK_AP_COLS_MAX, HeavisideAP and any other
    rank_approximation.  fused (SmoothAP, SupAP; CUDA fp32 / bf16 / fp16): one library call returns AP and its gradient
    (wv_rank_ap, csrc/rank_ap.hip) behind a torch.autograd.Function.  `fused = False` forces the plain path;
    `check_labels = False` promises 0 / 1 targets with a positive in every row (and a unit diagonal when square) and saves
    the check with its synchronise."""
    _kind = None            # the kernel's name for rank_approximation; None: plain path only

    def __init__(self, rank_approximation, return_type='1-mAP'):
        super().__init__()
        self.rank_approximation = rank_approximation
        self.return_type = return_type
        assert return_type in ["1-mAP", "1-AP", "AP", 'mAP']

    def general_forward(self, scores, target, verbose=False):
        mask = 1 - torch.eye(target.size(1), device=scores.device, dtype=scores.dtype)
        ap_score = []
        for idx in range(target.size(0)):
            pos_mask = target[idx].bool()
            query = scores[idx].view(1, -1) - scores[idx][pos_mask].view(-1, 1)                    # [positives, M]
            query = self.rank_approximation(query, target=pos_mask, general=True) * mask[pos_mask]
            rk = 1 + query.sum(-1)
            pos_rk = 1 + (query * pos_mask.view(1, -1)).sum(-1)
            ap_score.append((pos_rk / rk).sum(-1) / pos_mask.sum())
        return torch.stack(ap_score)

    def quick_forward(self, scores, target):
        eye = torch.eye(target.size(0), device=scores.device, dtype=scores.dtype)
        sim_diff = scores.unsqueeze(1) - scores.unsqueeze(2)                                       # [q, i, j] = S[q, j] - S[q, i]
        sim_diff_sigmoid = self.rank_approximation(sim_diff, target=target)
        sim_all_rk = torch.sum(sim_diff_sigmoid * (1.0 - eye.unsqueeze(0)), dim=-1) + 1
        sim_pos_rk = (torch.sum(sim_diff_sigmoid * (target - eye), dim=-1) + target) * target
        return (sim_pos_rk / sim_all_rk).sum(1) * (1 / target.sum(1))

    def _fused_params(self, general):
        kw = self.rank_approximation.keywords
        form = "general" if general else "quick"
        if self._kind == "smooth":
            return rank_ap_params("smooth", form, kw["tau"])
        delta, offset, start = kw["delta"], kw["offset"], kw["start"]
        if delta is None:                            # rho d + offset on every d > 0: a linear part that begins at 0
            delta = 0.0
        elif offset is None:
            offset = sup_offset(kw["tau"], delta, start)
        return rank_ap_params("sup", form, kw["tau"], kw["rho"], offset, delta, start)

    def _takes_fused(self, scores, target, general):
        if not (self._fusable(scores) and self._kind is not None):
            return False
        if not (1 <= scores.shape[0] <= RANK_AP_COLS_MAX and 1 <= scores.shape[1] <= RANK_AP_COLS_MAX):
            return False
        kw = self.rank_approximation.keywords
        if isinstance(kw["tau"], str) or (self._kind == "sup" and kw["delta"] is None and kw["offset"] is None):
            return False
        if not self.check_labels:
            return True
        ok = ((target == 0) | (target == 1)).all() & (target != 0).any(1).all()
        if not general:
            ok = ok & (target.diagonal() == 1).all()
        return bool(ok)

    def forward(self, scores, target, force_general=False, verbose=False):
        assert scores.shape == target.shape
        assert len(scores.shape) == 2

        general = force_general or scores.size(0) != scores.size(1)
        if self._takes_fused(scores, target, general):
            ap = self._fused(rank_ap, None, scores, target.to(device=scores.device, dtype=torch.float32), self._fused_params(general))
        elif general:
            ap = self._run_plain(partial(self.general_forward, verbose=verbose), scores, target)
        else:
            ap = self._run_plain(self.quick_forward, scores, target)

        if self.return_type == 'AP':
            return ap
        elif self.return_type == 'mAP':
            return ap.mean()
        elif self.return_type == '1-AP':
            return 1 - ap
        elif self.return_type == '1-mAP':
            return 1 - ap.mean()

    @property
    def my_repr(self):
        return f"return_type={self.return_type}"


class HeavisideAP(SmoothRankAP):
    """here for testing purposes: the exact rank, no gradient.  Always the plain path."""

    def __init__(self, **kwargs):
        super().__init__(partial(heaviside), **kwargs)

    def extra_repr(self):
        return self.my_repr


class SmoothAP(SmoothRankAP):
    _kind = "smooth"

    def __init__(self, tau=0.01, **kwargs):
        super().__init__(partial(tau_sigmoid, tau=tau), **kwargs)
        self.tau = tau

    def extra_repr(self):
        return f"tau={self.tau}, {self.my_repr}"


class SupAP(SmoothRankAP):
    """`loss: roadmap`'s ranking part (config/loss/roadmap.yaml: tau 0.01, rho 100, offset 1.44, delta 0.05)."""
    _kind = "sup"

    def __init__(self, tau=0.01, rho=100, offset=None, delta=0.05, start=0.5, **kwargs):
        super().__init__(partial(step_rank, tau=tau, rho=rho, offset=offset, delta=delta, start=start), **kwargs)
        self.tau = tau
        self.rho = rho
        self.offset = offset
        self.delta = delta

    def extra_repr(self):
        return f"tau={self.tau}, rho={self.rho}, offset={self.offset}, delta={self.delta}, {self.my_repr}"
