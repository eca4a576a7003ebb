"""Shared by tests/test_pair_losses_host.py and tests/test_gpu_pair_loss.py: seeded inputs of wv_pair_loss, a float64
restatement of the two losses written from their definitions (include/wvhash.h), and the error measure.
No test functions.  Everything is made on the host, once per case (functools caches), and never modified.

Shapes, the smallest where the kernel can go wrong: it owns 8 rows per workgroup and walks columns in tiles of 32, so
B = 1, 2, 7 / 8 / 9 (row block), 31 / 32 / 33 (column tile), 96 (the study's batch), 257 with two label words; D = 1, 3, 64,
65, 300, 512 (a thread owns columns d and d + 256: at 300 the second slot is partly used; the dot product runs four chains
with a tail).  Labels:
  dense     Bernoulli(0.08) tags, row 1 empty, rows 2 and 3 identical
  word2     80 classes, classes 0..63 cleared: hits lie in the second label word only
  identical every row the same non-empty set: HashNet's S0 = 0, SCH's pairs all `same`
  empty     no tag anywhere: HashNet's S1 = 0, SCH's pairs all `disjoint` (its second part is exactly 0)
  onehot    distinct one-hot rows on +-1 codes with n_bits = D: SCH's second part is exactly 0 while the first is not
"""
import collections
import functools

import torch

TOL = 5e-5          # the figure the project holds its fp32 twins to against reference-made goldens

Case = collections.namedtuple("Case", "B D C labels kind seed")
# kind -> (loss, apply_tanh, pre_scale, alpha, beta); n_bits = D
KINDS = {
    "sch_tanh": ("sch", True, 1.0, 0.3, 0.2),
    "sch_pre": ("sch", False, 1.0, 1.0, 0.1),
    "hashnet_s1": ("hashnet", True, 1.0, 0.1, 0.0),
    "hashnet_s3": ("hashnet", True, 3.0, 0.1, 0.0),
}


def _cases():
    shapes = [(1, 64, 38, "dense"), (2, 3, 38, "dense"), (7, 64, 20, "dense"), (8, 1, 20, "dense"), (9, 65, 38, "dense"),
              (31, 64, 38, "dense"), (32, 64, 38, "dense"), (33, 64, 38, "dense"), (96, 64, 38, "dense"),
              (257, 128, 80, "dense"), (40, 512, 38, "dense"), (33, 16, 80, "word2"), (24, 64, 38, "identical"),
              (24, 64, 38, "empty"), (9, 300, 38, "dense")]
    out = [Case(B, D, C, lab, kind, 1000 + 10 * i) for i, (B, D, C, lab) in enumerate(shapes) for kind in KINDS]
    out.append(Case(20, 64, 38, "onehot", "sch_pre", 2000))
    return out


CASES = _cases()
BIG_CASE = Case(2048, 64, 38, "dense", "sch_tanh", 3000)      # the row limit: 256 workgroups, 64 column tiles


def case_id(c):
    return f"{c.kind}-B{c.B}-D{c.D}-C{c.C}-{c.labels}"


def pack_bits(x):
    """[rows, n] (> 0 = set) -> int64 [rows, ceil(n / 64)], bit j of word w = x[:, 64 w + j]: what pack_labels makes"""
    rows, n = x.shape
    words = (n + 63) // 64
    b = torch.zeros((rows, words * 64), dtype=torch.int64)
    b[:, :n] = (x > 0).long()
    return (b.view(rows, words, 64) << torch.arange(64, dtype=torch.int64)).sum(2)


def make_labels(B, C, which, seed):
    g = torch.Generator().manual_seed(seed)
    lab = (torch.rand(B, C, generator=g) < 0.08).float()
    if which == "dense":
        if B > 1:
            lab[1] = 0
        if B > 3:
            lab[3] = lab[2]
    elif which == "word2":
        lab = (torch.rand(B, C, generator=g) < 0.15).float()
        lab[:, :64] = 0
        lab[0, 70] = lab[1, 70] = 1
    elif which == "identical":
        lab[:] = 0
        lab[:, [2, 5, 11]] = 1
    elif which == "empty":
        lab[:] = 0
    elif which == "onehot":
        lab = torch.eye(C)[:B].clone()
    return lab


Inputs = collections.namedtuple("Inputs", "e labels packed loss apply_tanh pre_scale nbits alpha beta")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The tensors and constants of a case (host, fp32 / int64): never modified by a test."""
    loss, apply_tanh, pre_scale, alpha, beta = KINDS[case.kind]
    g = torch.Generator().manual_seed(case.seed)
    e = 1.5 * torch.randn(case.B, case.D, generator=g)
    if case.labels == "onehot":
        e = torch.where(e >= 0, torch.ones_like(e), -torch.ones_like(e))
    elif not apply_tanh:
        e = torch.tanh(e)
    lab = make_labels(case.B, case.C, case.labels, case.seed + 1)
    return Inputs(e, lab, pack_bits(lab), loss, apply_tanh, pre_scale, float(case.D), alpha, beta)


def params_of(x):
    from wvhash.losses import pair_loss_params
    return pair_loss_params(x.loss, x.apply_tanh, x.pre_scale, x.nbits, x.alpha, x.beta)


def restate64(loss, e, labels, apply_tanh, pre_scale, nbits, alpha, beta):
    """The definitions of include/wvhash.h in float64, pair relations on integers -> (out float64 [3], grad float64 [B, D])"""
    e = e.double().detach().requires_grad_(True)
    L = (labels > 0).long()
    c = L @ L.t()
    n = L.sum(1)
    B = e.shape[0]
    u = pre_scale * e
    if apply_tanh:
        u = torch.tanh(u)
    G = u @ u.t()
    if loss == "sch":
        k = float(nbits)
        ni, nj = n[:, None].expand(B, B), n[None, :].expand(B, B)
        same = (c > 0) & (c == ni) & (c == nj)
        disjoint = c == 0
        S = torch.zeros(B, B, dtype=torch.float64)
        ok = (ni * nj) > 0
        S[ok] = c[ok].double() / (ni[ok] * nj[ok]).double().sqrt()
        lam = (1 - S) * k / 2
        lam[same] = 0.0
        lam_l = (lam - 3).clamp(min=0)
        lam_l[disjoint] = k / 2
        W_l = torch.ones(B, B, dtype=torch.float64)
        W_l[disjoint] = beta
        W_l[same] = 0.0
        W_u = torch.ones(B, B, dtype=torch.float64)
        W_u[disjoint] = 0.0
        W_u[same] = alpha
        H = (k - G) / 2
        sq1 = ((lam_l - H).clamp(min=0) * W_l).pow(2).sum()
        sq2 = ((H - lam).clamp(min=0) * W_u).pow(2).sum()
        # a part whose norm is 0 has gradient 0: sqrt is not differentiated there
        part1 = sq1.sqrt() / B ** 2 if float(sq1.detach()) > 0 else sq1 * 0
        part2 = sq2.sqrt() / B ** 2 if float(sq2.detach()) > 0 else sq2 * 0
    else:
        P = c > 0
        dp = alpha * G
        t = torch.logaddexp(dp, torch.zeros_like(dp)) - P.double() * dp
        S1 = int(P.sum())
        S0 = B * B - S1
        part1 = t[P].sum() / S1 if S1 else t.sum() * 0
        part2 = t[~P].sum() / S0 if S0 else t.sum() * 0
    total = part1 + part2
    (grad,) = torch.autograd.grad(total, e)
    return torch.stack([total.detach(), part1.detach(), part2.detach()]), grad


@functools.lru_cache(maxsize=None)
def reference(case):
    x = inputs(case)
    return restate64(x.loss, x.e, x.labels, x.apply_tanh, x.pre_scale, x.nbits, x.alpha, x.beta)


def scalar_err(got, want):
    """relative distance of a scalar; a reference of exactly 0 must be met exactly"""
    got, want = float(torch.as_tensor(got).detach()), float(want)
    if want == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - want) / abs(want)


def grad_err(got, want):
    """norm-wise: max |x - x64| / max |x64|; a zero reference must be met exactly"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert torch.isfinite(got).all(), "NaN or inf in the gradient"
    top = float(want.abs().max())
    diff = float((got - want).abs().max())
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top


def bf16_grad_slack(got, want):
    """The worst element of a bf16 gradient over its allowance (met when <= 0); want: the plain path's fp32 gradient.
    The fused gradient is rounded to bf16 at the end: against the plain gradient rounded the same way, every element
    within one bf16 last place (2^-7 of its value) plus what TOL of the largest value can move an element before rounding"""
    got, want = got.double(), want.to(got.dtype).double()
    slack = (got - want).abs() - (2.0 ** -7 * want.abs() + TOL * float(want.abs().max()))
    return float(slack.max())


def check(out, grad, ref_out, ref_grad, what):
    """out [3] and grad against a float64 reference within TOL; prints the figures first"""
    errs = [scalar_err(out[i], ref_out[i]) for i in range(3)]
    ge = grad_err(grad, ref_grad) if grad is not None else 0.0
    print(f"{what}: loss {errs[0]:.2e} parts {errs[1]:.2e} {errs[2]:.2e} grad {ge:.2e}")
    assert max(errs) <= TOL and ge <= TOL, (what, errs, ge)
    return max(errs), ge
