"""SmoothRankAP / SmoothAP / SupAP / HeavisideAP (wvhash/losses.py) without a GPU: the plain PyTorch path, the host twin
wv_rank_ap_cpu and the float64 restatement of tests/rank_ap_cases.py against the reference-made goldens
(tests/golden/rank_ap_golden.npz, make_golden_rank_ap.py); the twin against the restatement on every case of the kernel's
list; return types, force_general and the choice between the two forms; the NaN of a row without a positive and the other
inputs only the plain path takes; the modules' surface; the entry points' argument gate; one train_step through the
score-matrix branch of _criterion_loss."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rank_ap_cases as C
from wvhash import _lib
from wvhash import losses as L


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rank_ap_golden.npz"))


def _errs(ap, grad, want_ap, want_grad):
    return max(C.scalar_err(ap[q], want_ap[q]) for q in range(len(want_ap))), C.grad_err(grad, want_grad)


def _plain(case, scores, target, dtype, return_type="AP"):
    """The module's plain path (CPU tensors always take it) -> (value, gradient of its sum)"""
    s = scores.to(dtype).detach().clone().requires_grad_(True)
    val = C.module_of(case, return_type)(s, target, force_general=case.form == "general")
    val.sum().backward()
    return val.detach(), s.grad


@pytest.mark.parametrize("case", C.GOLDEN_CASES, ids=C.case_id)
def test_plain_path_twin_and_restatement_meet_the_reference_made_goldens(golden, case):
    assert list(golden["cases"]) == [C.case_id(c) for c in C.GOLDEN_CASES]
    x = C.inputs(case)
    tag = C.case_id(case)
    # the fixture was made from the inputs the builder makes today
    assert np.array_equal(golden[f"{case.name}/scores"], x.scores.numpy())
    assert np.array_equal(golden[f"{case.name}/target"], x.target.numpy().astype(np.uint8))
    want_ap, want_grad = torch.from_numpy(golden[f"{tag}/ap"]), torch.from_numpy(golden[f"{tag}/grad"])
    assert want_ap.dtype == torch.float64 and want_grad.shape == x.scores.shape
    # SupAP's offset=None: the reference forms start + sigmoid(delta) in fp32, this package in double -- half an fp32 last
    # place of the offset (6e-8), which every linear-branch R carries into rk and prk: an fp32 last place, 2^-23, bounds it
    auto = 2.0 ** -23 if case.kind == "sup_auto" else 0.0
    for dtype, tol in ((torch.float32, C.TOL), (torch.float64, max(1e-9, auto))):
        ea, eg = _errs(*_plain(case, x.scores, x.target, dtype), want_ap, want_grad)
        print(f"plain {dtype}: ap {ea:.2e} grad {eg:.2e}")
        assert ea <= tol and eg <= tol
    ea, eg = _errs(*L.rank_ap_host(x.scores, x.target, C.params_of(x)), want_ap, want_grad)
    print(f"twin: ap {ea:.2e} grad {eg:.2e}")
    assert ea <= C.TOL and eg <= C.TOL
    # the float64 restatement the GPU tests use as their reference describes the same function
    ea, eg = _errs(*C.reference(case), want_ap, want_grad)
    print(f"restatement: ap {ea:.2e} grad {eg:.2e}")
    assert ea <= max(1e-12, auto) and eg <= max(1e-12, auto)


@pytest.mark.parametrize("case", C.CASES + C.BIG_CASES, ids=C.case_id)
def test_twin_meets_the_restatement(case):
    x = C.inputs(case)
    ref_ap, ref_grad = C.reference(case)
    ap, grad = L.rank_ap_host(x.scores, x.target, C.params_of(x))
    assert ap.dtype == torch.float32 and ap.shape == (case.B,) and grad.shape == x.scores.shape
    C.check(ap, grad, ref_ap, ref_grad, "twin")
    ap2, none = L.rank_ap_host(x.scores, x.target, C.params_of(x), want_grad=False)
    assert none is None and torch.equal(ap2, ap)
    if case.name == "selfonly":
        assert float(ap[0]) == 1.0 and float(grad[0].abs().max()) == 0.0
    if case.name == "allpos":
        assert torch.equal(ap, torch.ones(case.B)) and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("case", [c for c in C.CASES if c.M <= 130], ids=C.case_id)
def test_plain_path_meets_the_restatement(case):
    """fp32 within TOL, float64 to 1e-11; a zero gradient (all-ones target) is met to rounding of the O(1) terms that cancel"""
    x = C.inputs(case)
    ref_ap, ref_grad = C.reference(case)
    for dtype, tol, eps in ((torch.float32, C.TOL, 2.0 ** -23), (torch.float64, 1e-11, 2.0 ** -52)):
        ap, grad = _plain(case, x.scores, x.target, dtype)
        assert ap.dtype == dtype
        if case.name == "allpos":
            assert float(ref_grad.abs().max()) == 0.0 and float(grad.abs().max()) <= 64 * eps / x.tau
            assert max(C.scalar_err(ap[q], ref_ap[q]) for q in range(case.B)) <= tol
        else:
            ea, eg = _errs(ap, grad, ref_ap, ref_grad)
            assert ea <= tol and eg <= tol, (dtype, ea, eg)


def test_the_cases_reach_every_branch():
    """All three SupAP branches, pairs outside the sigmoid's clamp, and (duplicated columns) d = 0 between two columns"""
    for name in ("63x63", "257x257", "5x130", "16x50", "batch96"):
        census = C.branch_census(next(c for c in C.CASES if c.name == name and c.kind == "sup"))
        assert min(census[k] for k in ("linear", "shifted", "sigmoid", "clamped")) > 0, (name, census)
    assert C.branch_census(next(c for c in C.CASES if c.name == "dups" and c.kind == "sup"))["zero"] > 0
    assert C.branch_census(C.BIG_CASES[1])["shifted"] > 0


def test_the_two_forms_differ_on_a_multi_hot_target():
    case = next(c for c in C.CASES if c.name == "nonsym" and c.kind == "smooth" and c.form == "quick")
    quick, general = C.reference(case)[0], C.reference(case._replace(form="general"))[0]
    assert float((quick - general).abs().max()) > 0.05


def test_return_types_force_general_and_the_choice_of_form(monkeypatch):
    case = next(c for c in C.CASES if c.name == "16x50" and c.kind == "sup")
    square = next(c for c in C.CASES if c.name == "65x65" and c.kind == "sup" and c.form == "quick")
    seen = []
    for name in ("quick_forward", "general_forward"):
        inner = getattr(L.SmoothRankAP, name)
        monkeypatch.setattr(L.SmoothRankAP, name, lambda self, *a, _n=name, _f=inner, **k: seen.append(_n) or _f(self, *a, **k))
    xs, xr = C.inputs(square), C.inputs(case)
    ap = C.module_of(square, "AP")(xs.scores, xs.target)
    assert seen == ["quick_forward"] and ap.shape == (65,)
    forced = C.module_of(square, "AP")(xs.scores, xs.target, force_general=True)
    rect = C.module_of(case, "AP")(xr.scores, xr.target, verbose=True)
    assert seen == ["quick_forward", "general_forward", "general_forward"] and rect.shape == (16,)
    assert not torch.allclose(ap, forced)
    for rt, want in (("mAP", ap.mean()), ("1-AP", 1 - ap), ("1-mAP", 1 - ap.mean())):
        got = C.module_of(square, rt)(xs.scores, xs.target)
        assert got.shape == want.shape and torch.equal(got, want), rt
    assert C.module_of(square).return_type == "AP" and L.SupAP().return_type == "1-mAP"
    with pytest.raises(AssertionError):
        L.SupAP(return_type="map")
    with pytest.raises(AssertionError):
        L.SupAP()(xr.scores, xr.target[:, :49])
    with pytest.raises(AssertionError):
        L.SupAP()(xr.scores[0], xr.target[0])


def test_module_surface():
    s = L.SupAP()
    assert (s.tau, s.rho, s.offset, s.delta, s.return_type) == (0.01, 100, None, 0.05, "1-mAP")
    assert s.extra_repr() == "tau=0.01, rho=100, offset=None, delta=0.05, return_type=1-mAP"
    assert repr(L.SmoothAP(tau=0.02, return_type="AP")) == "SmoothAP(tau=0.02, return_type=AP)"
    assert repr(L.HeavisideAP()) == "HeavisideAP(return_type=1-mAP)"
    assert L.SmoothAP().tau == 0.01 and L.SmoothAP().my_repr == "return_type=1-mAP"
    for m in (s, L.SmoothAP(), L.HeavisideAP(), L.SmoothRankAP(L.tau_sigmoid)):
        assert isinstance(m, L.SmoothRankAP) and not hasattr(m, "takes_embeddings")      # train_step sends the score matrix
        assert (m.fused, m.check_labels) == (True, True) and list(m.parameters()) == [] and len(m.state_dict()) == 0
    kw = L.SupAP(tau=0.02, rho=10.0, offset=1.44, delta=0.1, start=0.25).rank_approximation.keywords
    assert kw == dict(tau=0.02, rho=10.0, offset=1.44, delta=0.1, start=0.25)
    assert abs(L.sup_offset(0.01, 0.05, 0.5) - (0.5 + 1 / (1 + np.exp(-5.0)))) < 1e-15


def test_heaviside_ap_is_the_exact_ap_and_has_no_gradient():
    g = torch.Generator().manual_seed(4)
    scores = torch.randn(6, 40, generator=g).requires_grad_(True)
    target = (torch.rand(6, 40, generator=g) < 0.3).float()
    target[:, 0] = 1
    ap = L.HeavisideAP(return_type="AP")(scores, target)
    for q in range(6):
        order = torch.argsort(scores[q].detach(), descending=True)
        rel = target[q][order]
        prec = torch.cumsum(rel, 0) / torch.arange(1, 41)
        assert abs(float(ap[q].detach()) - float((prec * rel).sum() / rel.sum())) < 1e-6
    ap.sum().backward()
    assert scores.grad is None or float(scores.grad.abs().max()) == 0.0


def test_plain_path_takes_what_the_fused_path_does_not():
    """CPU tensors, fp64, bf16 on the host (widened: an fp32 value, a bf16 gradient), targets that are not 0 / 1, a row
    without a positive (the reference's NaN, in that row only), a tau string, delta=None; autocast does not reach in."""
    case = next(c for c in C.CASES if c.name == "16x50" and c.kind == "sup")
    x = C.inputs(case)
    m = C.module_of(case, "AP")
    want = m(x.scores, x.target)
    assert want.device.type == "cpu" and want.dtype == torch.float32
    sb = x.scores.bfloat16().requires_grad_(True)
    got = m(sb, x.target)
    got.sum().backward()
    assert got.dtype == torch.float32 and sb.grad.dtype == torch.bfloat16
    assert torch.equal(got, m(x.scores.bfloat16().float(), x.target))
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert torch.equal(m(x.scores, x.target), want)
    assert m(x.scores.double(), x.target).dtype == torch.float64
    assert torch.equal(m(x.scores, 2.5 * x.target), want)                  # general form: any non-zero entry is a positive
    assert torch.equal(m(x.scores, x.target.bool()), want)
    empty = x.target.clone()
    empty[3] = 0
    out = m(x.scores, empty)
    assert torch.isnan(out[3]) and torch.isfinite(out[[0, 1, 2] + list(range(4, 16))]).all()
    sq = C.inputs(next(c for c in C.CASES if c.name == "65x65" and c.kind == "sup" and c.form == "quick"))
    holed = sq.target.clone()
    holed[:, 2] = 0                                                         # column 2 relevant to nobody, row 2 included
    assert torch.isfinite(L.SupAP(return_type="AP")(sq.scores, holed)).all()
    # two temperatures: 'n_p'; both equal to tau give tau's numbers
    assert torch.equal(L.SupAP(tau="0.01_0.01", offset=1.44, return_type="AP")(x.scores, x.target),
                       L.SupAP(tau=0.01, offset=1.44, return_type="AP")(x.scores, x.target))
    assert not torch.equal(L.SupAP(tau="0.05_0.01", offset=1.44, return_type="AP")(x.scores, x.target), want)
    # delta=None: rho d + offset on every d > 0, which is delta = 0 of the library
    lin = L.SupAP(tau=0.01, rho=100.0, offset=1.44, delta=None, return_type="AP")
    t_ap, _ = L.rank_ap_host(x.scores, x.target, lin._fused_params(True))
    assert max(C.scalar_err(t_ap[q], lin(x.scores, x.target).double()[q]) for q in range(16)) <= C.TOL
    with pytest.raises(TypeError):
        L.SupAP(delta=None)(x.scores, x.target)                            # offset=None too: as in the reference


@pytest.mark.parametrize("name, form", [("16x50", "general"), ("65x65", "quick")])
def test_fused_function_over_the_host_twin(name, form):
    """The autograd Function of the modules' fused path, run over rank_ap_host: AP and gradient through a grad_output that
    differs row by row against the plain path on the same fp32 input; a bf16 input gets a bf16 gradient; with want=False
    nothing is saved and the value has the same bits."""
    case = next(c for c in C.CASES if c.name == name and c.kind == "sup" and c.form == form)
    x = C.inputs(case)
    params = C.params_of(x)
    weights = torch.linspace(0.5, 2.0, case.B)
    s = x.scores.clone().requires_grad_(True)
    ap = L._FusedLoss.apply(L.rank_ap_host, None, s, x.target, params, True)
    (weights * ap).sum().backward()
    wide = x.scores.clone().requires_grad_(True)
    ref = C.module_of(case, "AP")(wide, x.target, force_general=form == "general")
    (weights * ref).sum().backward()
    ea, eg = _errs(ap, s.grad, ref.detach().double(), wide.grad.double())
    print(f"{name} {form}: ap {ea:.2e} grad {eg:.2e}")
    assert ap.shape == (case.B,) and ap.dtype == torch.float32 and s.grad.dtype == torch.float32
    assert ea <= C.TOL and eg <= C.TOL
    sb = x.scores.bfloat16().requires_grad_(True)
    L._FusedLoss.apply(L.rank_ap_host, None, sb, x.target, params, True).sum().backward()
    assert sb.grad.dtype == torch.bfloat16 and sb.grad.shape == sb.shape
    quiet = L._FusedLoss.apply(L.rank_ap_host, None, s, x.target, params, False)
    assert quiet.grad_fn.saved_tensors == ()
    assert torch.equal(quiet.detach().view(torch.int32), ap.detach().view(torch.int32))


def test_train_step_reaches_the_score_matrix_branch():
    from wvhash.engine import train_step
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 8))
    crit = L.SupAP(offset=1.44)
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(10, 3, 2, 2, generator=g), C.multi_hot(10, 3)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    before = net[1].weight.detach().clone()
    logs = train_step(net, x, y, [(crit, 1.0)], [opt], autocast_dtype=None)
    assert 0.0 < logs["SupAP"] < 1.0 and not torch.equal(net[1].weight.detach(), before)
    with torch.no_grad():
        emb = net(x)
        want = float(crit(emb @ emb.t(), ((y @ y.t()) > 0).float()))
    assert abs(want - train_step(net, x, y, [(crit, 1.0)], [opt], autocast_dtype=None)["SupAP"]) < 1e-6


def _gate(gpu, scores, target, B, M, params, ap, ws=None, ws_bytes=0):
    lib = _lib.load()
    if gpu:
        return lib.wv_rank_ap(scores, target, B, M, params, ap, None, ws, ws_bytes, None)
    return lib.wv_rank_ap_cpu(scores, target, B, M, params, ap, None)


@pytest.mark.parametrize("gpu", [False, True], ids=["twin", "kernel"])
def test_argument_gate_answers_before_any_pointer_is_read(gpu):
    lib = _lib.load()
    one = ctypes.c_void_p(16)                     # never dereferenced: every call below is refused first
    ok = ctypes.byref(L.rank_ap_params("sup", "general"))
    big = 1 << 40
    name = b"rank_ap:" if gpu else b"rank_ap_cpu:"

    def call(scores=one, target=one, B=8, M=16, params=ok, ap=one, ws=one, ws_bytes=big):
        return _gate(gpu, scores, target, B, M, params, ap, ws, ws_bytes)

    for kw, word in ((dict(scores=None), b"scores is null"), (dict(target=None), b"target is null"),
                     (dict(params=None), b"params is null"), (dict(ap=None), b"ap is null"), (dict(B=0), b"B=0"), (dict(M=0), b"M=0"),
                     (dict(params=ctypes.byref(L.rank_ap_params(2, "general"))), b"kind=2"),
                     (dict(params=ctypes.byref(L.rank_ap_params("sup", 2))), b"form=2"),
                     (dict(params=ctypes.byref(L.rank_ap_params("sup", "quick"))), b"square"),
                     (dict(params=ctypes.byref(L.rank_ap_params("sup", "general", tau=0.0))), b"tau=0"),
                     (dict(params=ctypes.byref(L.rank_ap_params("smooth", "general", tau=float("nan")))), b"tau=nan")):
        assert call(**kw) == -22, kw
        msg = lib.wv_last_error()
        assert msg.startswith(name) and word in msg, (kw, msg)
    assert call(M=4097) == -95 and b"M=4097 above WV_RANK_AP_COLS_MAX=4096" in lib.wv_last_error()
    assert call(B=4097) == -95 and b"B=4097 above WV_RANK_AP_COLS_MAX=4096" in lib.wv_last_error()
    assert _lib.WV_RANK_AP_COLS_MAX == 4096
    if gpu:
        q, g = _lib.WV_RANK_AP_QUICK, _lib.WV_RANK_AP_GENERAL
        assert lib.wv_rank_ap_workspace_bytes(8, 16, g) == 8 * 1 * 8 and lib.wv_rank_ap_workspace_bytes(8, 65, g) == 8 * 2 * 8
        assert lib.wv_rank_ap_workspace_bytes(65, 65, q) == 2 * 65 * 2 * 8 and lib.wv_rank_ap_workspace_bytes(0, 16, g) == 0
        assert call(ws=None) == -22 and b"workspace is null" in lib.wv_last_error()
        assert call(ws_bytes=63) == -22 and b"workspace" in lib.wv_last_error()


def test_wrapper_gate():
    s, t = torch.randn(6, 8), torch.ones(6, 8)
    p = L.rank_ap_params("smooth", "general")
    with pytest.raises(ValueError, match="rank_ap_host: scores: expected dtype torch.float32"):
        L.rank_ap_host(s.double(), t, p)
    with pytest.raises(ValueError, match="rank_ap_host: target: expected shape"):
        L.rank_ap_host(s, t[:5], p)
    with pytest.raises(ValueError, match="rank_ap_host: target: expected dtype torch.float32"):
        L.rank_ap_host(s, t.bool(), p)
    with pytest.raises(ValueError, match="rank_ap: scores: expected a tensor on a cuda device"):
        L.rank_ap(s, t, p)
    with pytest.raises(ValueError, match="params: expected a RankApParams"):
        L.rank_ap_host(s, t, {"kind": 0})
    with pytest.raises(ValueError, match="square"):
        L.rank_ap_host(s, t, L.rank_ap_params("smooth", "quick"))
    with pytest.raises(_lib.WvhashUnsupported, match="M=4097"):
        L.rank_ap_host(torch.zeros(1, 4097), torch.ones(1, 4097), p)
    ap, grad = L.rank_ap_host(s.t().contiguous().t(), t, p)               # a strided view is copied, not misread
    assert torch.equal(ap, L.rank_ap_host(s, t, p)[0]) and grad.shape == s.shape
    half = s.bfloat16()
    assert torch.equal(L.rank_ap_host(half, t, p)[0], L.rank_ap_host(half.float(), t, p)[0])
