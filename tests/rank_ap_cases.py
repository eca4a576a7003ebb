"""Shared by tests/test_rank_ap_host.py, tests/test_gpu_rank_ap.py and tests/golden/make_golden_rank_ap.py: seeded inputs
of wv_rank_ap, a float64 restatement of SmoothAP / SupAP written from their definitions (include/wvhash.h) with explicit
loops over the queries and their positives, and the error measure (TOL, scalar_err, grad_err and bf16_grad_slack are pair_loss_cases.py's).
No test functions.  Everything is made on the host, once per case (functools caches), and never modified.

Shapes, the smallest where the kernel can go wrong: a bit row is made of 64-column words and a wave's lanes stride the
columns by 64, so M = 1, 2, 63 / 64 / 65 and 255 / 256 / 257 (four words and a fifth of one bit), the rectangular 5 x 130 and
16 x 50 (general form only), and 2 x 4096 at the column limit (eight waves share 400 positives, a thread owns 8 columns).
Square cases run in both forms.  Targets:
  labels   T = (L L^t > 0) of 15 %-dense multi-hot labels with no empty row (rectangular: T[q, q % M] set): unit diagonal
  nonsym   independent Bernoulli(0.2) entries, unit diagonal: T[i, j] != T[j, i] -- the quick form weighs by T[i, j], not T[q, j]
  selfonly labels, but row 0 has the single positive 0 whose score beats every other by more than 50 tau: AP exactly 1, gradient 0
  allpos   all ones: every f_i = 1, gradient exactly 0
  dups     labels; columns 3, 7 and 11 carry one score in every row (d = 0 between two different columns)
Scores are inner products of unit vectors in 8 dimensions (fp32), so d spans [-2, 2]: with tau = 0.01 and delta = 0.05 all
three SupAP branches and |d| / tau > 50 occur in every case of 63 columns or more (branch_census() counts them).

Input condition, asserted by inputs(): SupAP with offset = 1.44 jumps by about 0.05 at d = delta, so an fp32 `d > delta` may
differ from float64 on a pair within rounding of delta.  No case may have a pair (q, i in P, j) with |d - delta| <= 2^-24, d
formed in float64 from the fp32 scores; the seeds below were picked so.  The sign of d is exact in fp32: d = 0 needs none."""
import collections
import functools

import numpy as np
import torch

from pair_loss_cases import TOL, bf16_grad_slack, grad_err, scalar_err  # noqa: F401

COLS_MAX = 4096
DELTA = 0.05
KINDS = {
    "smooth": dict(kind="smooth", tau=0.01, rho=0.0, offset=0.0, delta=0.0, start=0.0),
    "sup": dict(kind="sup", tau=0.01, rho=100.0, offset=1.44, delta=DELTA, start=0.5),          # config/loss/roadmap.yaml
    "sup_auto": dict(kind="sup", tau=0.02, rho=10.0, offset=None, delta=DELTA, start=0.5),      # offset = start + sigmoid(delta)
}

Case = collections.namedtuple("Case", "name B M target kind form seed")


def _cases():
    shapes = [("1x1", 1, 1, "labels"), ("2x2", 2, 2, "labels"), ("63x63", 63, 63, "labels"), ("64x64", 64, 64, "labels"),
              ("65x65", 65, 65, "labels"), ("255x255", 255, 255, "labels"), ("256x256", 256, 256, "labels"),
              ("257x257", 257, 257, "labels"), ("5x130", 5, 130, "labels"), ("16x50", 16, 50, "labels"),
              ("nonsym", 70, 70, "nonsym"), ("selfonly", 70, 70, "selfonly"), ("allpos", 66, 66, "allpos"),
              ("dups", 70, 70, "dups"), ("batch96", 96, 96, "labels")]
    seeds = {"255x255": 4105}                         # the others: 100 + position; all checked by inputs()
    out = []
    for n, (name, B, M, target) in enumerate(shapes):
        for kind in ("smooth", "sup") + (("sup_auto",) if name == "batch96" else ()):
            for form in (("quick", "general") if B == M else ("general",)):
                out.append(Case(name, B, M, target, kind, form, seeds.get(name, 100 + n)))
    return out


CASES = _cases()
BIG_CASES = [Case("2x4096", 2, COLS_MAX, "bernoulli", kind, "general", 900) for kind in ("smooth", "sup")]
# what the reference is run on for tests/golden/rank_ap_golden.npz (it squeezes size-1 dimensions away: no 1 x 1 there)
GOLDEN_CASES = [c for c in CASES if c.name in ("2x2", "65x65", "16x50", "5x130", "nonsym", "dups", "batch96")]


def case_id(c):
    return f"{c.name}-{c.kind}-{c.form}"


def _unit(rows, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(rows, 8, generator=g)
    return e / e.norm(dim=1, keepdim=True)


def multi_hot(rows, seed, classes=10, p=0.15):
    """multi-hot labels [rows, classes] with no empty row"""
    g = torch.Generator().manual_seed(seed)
    L = (torch.rand(rows, classes, generator=g) < p).float()
    L[L.sum(1) == 0, 0] = 1
    return L


def make_target(B, M, which, seed):
    g = torch.Generator().manual_seed(seed)
    if which == "allpos":
        return torch.ones(B, M)
    if which == "bernoulli":
        T = (torch.rand(B, M, generator=g) < 0.1).float()
        T[:, 0] = 1
        return T
    if which == "nonsym":
        T = (torch.rand(B, M, generator=g) < 0.2).float()
        T.fill_diagonal_(1)
        return T
    L = multi_hot(max(B, M), seed)
    T = ((L[:B] @ L[:M].t()) > 0).float()
    T[torch.arange(B), torch.arange(B) % M] = 1
    if which == "selfonly":
        T[0] = 0
        T[0, 0] = 1
    return T


Inputs = collections.namedtuple("Inputs", "scores target kind form tau rho offset delta start")


def near_delta(scores, target, delta=DELTA):
    """pairs (q, i in P, j) with |d - delta| <= 2^-24, d in float64 from the fp32 scores"""
    S = scores.double().numpy()
    T = target.numpy() != 0
    count = 0
    for q in range(S.shape[0]):
        d = S[q][None, :] - S[q][T[q]][:, None]
        count += int((np.abs(d - delta) <= 2.0 ** -24).sum())
    return count


@functools.lru_cache(maxsize=None)
def _tensors(name, B, M, target, seed):
    scores = _unit(B, seed) @ (_unit(B, seed) if B == M else _unit(M, seed + 1)).t()
    if target == "dups":
        scores[:, 7] = scores[:, 3]
        scores[:, 11] = scores[:, 3]
    if target == "selfonly":
        scores[0, 1:] *= 0.3                          # S[0, 0] = 1 beats the rest by 0.7 = 70 tau at least
        scores[0, 0] = 1.0
    T = make_target(B, M, target, seed + 2)
    assert near_delta(scores, T) == 0, f"{name}: a pair lies within 2^-24 of delta: pick another seed"
    return scores, T


def inputs(case):
    """The tensors and constants of a case (host, fp32): never modified by a test."""
    scores, T = _tensors(case.name, case.B, case.M, case.target, case.seed)
    k = KINDS[case.kind]
    offset = k["offset"]
    if offset is None:
        offset = k["start"] + float(_sigmoid64(np.array(k["delta"]), k["tau"])[0])
    return Inputs(scores, T, k["kind"], case.form, k["tau"], k["rho"], offset, k["delta"], k["start"])


def params_of(x):
    from wvhash.losses import rank_ap_params
    return rank_ap_params(x.kind, x.form, x.tau, x.rho, x.offset, x.delta, x.start)


def module_of(case, return_type="AP"):
    """The wvhash.losses module that computes this case (form chosen by force_general at the call)"""
    from wvhash import losses as L
    k = KINDS[case.kind]
    if k["kind"] == "smooth":
        return L.SmoothAP(tau=k["tau"], return_type=return_type)
    return L.SupAP(tau=k["tau"], rho=k["rho"], offset=k["offset"], delta=k["delta"], start=k["start"], return_type=return_type)


def _sigmoid64(d, tau):
    x = -d / tau
    inside = (x >= -50) & (x <= 50)
    s = 1.0 / (1.0 + np.exp(np.clip(x, -50, 50)))
    return s, np.where(inside, s * (1 - s) / tau, 0.0)


def _term64(kind, d, tgt, tau, rho, offset, delta, start):
    """R(d) and R'(d) for a vector of pairs"""
    s, ds = _sigmoid64(d, tau)
    if kind == "smooth":
        return s, ds
    R = np.where(d > 0, np.where(d > delta, rho * (d - delta) + offset, start + s), s)
    dR = np.where((d > 0) & (d > delta), rho, ds)
    return np.where(tgt, (d >= 0).astype(np.float64), R), np.where(tgt, 0.0, dR)


def restate64(kind, form, scores, target, tau, rho, offset, delta, start):
    """The definitions in float64: a loop over the queries, a loop over each query's positives, the columns as a vector
    -> (ap float64 [B], grad float64 [B, M]); a row without a positive: ap 0, grad 0"""
    S = scores.double().numpy()
    T = target.numpy() != 0
    B, M = S.shape
    quick = form == "quick"
    assert not quick or B == M
    LM = (T.astype(np.int64) @ T.astype(np.int64).T) > 0 if quick else None
    ap, grad = np.zeros(B), np.zeros((B, M))
    for q in range(B):
        P = np.flatnonzero(T[q])
        n = len(P)
        for i in P:
            d = S[q] - S[q, i]
            tgt = (LM[i] & T[q]) if quick else T[q]
            w = (T[i] if quick else T[q]).astype(np.float64)
            R, dR = _term64(kind, d, tgt, tau, rho, offset, delta, start)
            others = np.arange(M) != i
            rk = 1.0 + R[others].sum()
            prk = 1.0 + (R * w)[others].sum()
            f = prk / rk
            ap[q] += f / n
            g = np.where(others, (w - f) / (rk * n) * dR, 0.0)
            grad[q] += g
            grad[q, i] -= g.sum()
    return torch.from_numpy(ap), torch.from_numpy(grad)


@functools.lru_cache(maxsize=None)
def reference(case):
    x = inputs(case)
    return restate64(x.kind, x.form, x.scores, x.target, x.tau, x.rho, x.offset, x.delta, x.start)


def branch_census(case):
    """Pairs (q, i in P, j not in P) of a case -- non-target pairs in either form -- by SupAP branch, those outside the
    sigmoid's clamp, and those with d = 0"""
    x = inputs(case)
    S, T = x.scores.double().numpy(), x.target.numpy() != 0
    out = collections.Counter()
    for q in range(case.B):
        for i in np.flatnonzero(T[q]):
            d = (S[q] - S[q, i])[~T[q]]
            out["linear"] += int((d > x.delta).sum())
            out["shifted"] += int(((d > 0) & (d <= x.delta)).sum())
            out["sigmoid"] += int((d <= 0).sum())
            out["clamped"] += int((np.abs(d) / x.tau > 50).sum())
            out["zero"] += int((d == 0).sum())
    return out


def check(ap, grad, ref_ap, ref_grad, what):
    """ap [B] (relative, per row) and grad (norm-wise) against a float64 reference within TOL; prints the figures first"""
    ea = max(scalar_err(ap[q], ref_ap[q]) for q in range(len(ref_ap)))
    eg = grad_err(grad, ref_grad) if grad is not None else 0.0
    print(f"{what}: ap {ea:.2e} grad {eg:.2e}")
    assert ea <= TOL and eg <= TOL, (what, ea, eg)
    return ea, eg
