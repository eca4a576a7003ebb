"""wv_rank_ap on the GPU: the kernel's ap / grad against the float64 restatement and the host twin on every case of
tests/rank_ap_cases.py (bit-word edges M = 1, 2, 63 / 64 / 65, 255 / 256 / 257, rectangular inputs, both kinds, both forms
where square, a non-symmetric target, rows whose AP is exactly 1 and whose gradient is exactly 0, duplicated scores), the
column limit and the refusal beyond it, run-to-run bits, grad = NULL, a side stream, the fused autograd Function against
the plain path (fp32 and bf16 inputs, non-unit grad_output, no_grad), and six train_steps on DINOHashBaseline under SupAP."""
import pytest
import torch

import rank_ap_cases as C
import single_band_cases as SB
from wvhash import _lib
from wvhash import losses as L

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(x, want_grad=True):
    return L.rank_ap(x.scores.cuda(), x.target.cuda(), C.params_of(x), want_grad=want_grad)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernel_against_float64_and_the_twin(case):
    x = C.inputs(case)
    ref_ap, ref_grad = C.reference(case)
    ap, grad = _run(x)
    assert ap.dtype == torch.float32 and grad.dtype == torch.float32 and ap.shape == (case.B,) and grad.shape == x.scores.shape
    C.check(ap.cpu(), grad.cpu(), ref_ap, ref_grad, "kernel vs float64")
    t_ap, t_grad = L.rank_ap_host(x.scores, x.target, C.params_of(x))
    C.check(ap.cpu(), grad.cpu(), t_ap.double(), t_grad.double(), "kernel vs twin")
    # the same call again: the same bits; without the gradient: the same ap bits
    ap2, grad2 = _run(x)
    assert torch.equal(_bits(ap), _bits(ap2)) and torch.equal(_bits(grad), _bits(grad2))
    ap3, none = _run(x, want_grad=False)
    assert none is None and torch.equal(_bits(ap), _bits(ap3))


@pytest.mark.parametrize("case", [c for c in C.CASES if c.name in ("selfonly", "allpos")], ids=C.case_id)
def test_rows_that_are_exact(case):
    """A row whose only positive beats every other column by more than 50 tau: AP exactly 1 and gradient exactly 0 (every
    pair is outside the sigmoid's clamp).  An all-ones target: f_i = 1 for every positive, so every coefficient is 0."""
    ap, grad = _run(C.inputs(case))
    rows = slice(0, 1) if case.name == "selfonly" else slice(None)
    assert torch.equal(ap[rows].cpu(), torch.ones_like(ap[rows]).cpu())
    assert float(grad[rows].abs().max()) == 0.0
    assert float(grad.abs().max()) > 0.0 or case.name == "allpos"


def test_a_row_without_a_positive_gives_zero():
    case = next(c for c in C.CASES if c.name == "16x50" and c.kind == "sup")
    x = C.inputs(case)
    T = x.target.clone()
    T[3] = 0
    ap, grad = L.rank_ap(x.scores.cuda(), T.cuda(), C.params_of(x))
    assert float(ap[3]) == 0.0 and float(grad[3].abs().max()) == 0.0 and torch.isfinite(ap).all() and torch.isfinite(grad).all()
    ref_ap, ref_grad = C.restate64(x.kind, x.form, x.scores, T, x.tau, x.rho, x.offset, x.delta, x.start)
    C.check(ap.cpu(), grad.cpu(), ref_ap, ref_grad, "kernel vs float64, row 3 empty")


@pytest.mark.parametrize("case", C.BIG_CASES, ids=C.case_id)
def test_column_limit_4096(case):
    x = C.inputs(case)
    ref_ap, ref_grad = C.reference(case)
    ap, grad = _run(x)
    C.check(ap.cpu(), grad.cpu(), ref_ap, ref_grad, "kernel vs float64, 2 x 4096")
    t_ap, t_grad = L.rank_ap_host(x.scores, x.target, C.params_of(x))
    C.check(ap.cpu(), grad.cpu(), t_ap.double(), t_grad.double(), "kernel vs twin, 2 x 4096")
    ap2, grad2 = _run(x)
    assert torch.equal(_bits(ap), _bits(ap2)) and torch.equal(_bits(grad), _bits(grad2))


def test_refusal_above_the_limit():
    assert L.RANK_AP_COLS_MAX == C.COLS_MAX
    p = L.rank_ap_params("sup", "general", 0.01, 100.0, 1.44, 0.05, 0.5)
    for shape in ((1, C.COLS_MAX + 1), (C.COLS_MAX + 1, 2)):
        with pytest.raises(_lib.WvhashUnsupported, match="WV_RANK_AP_COLS_MAX"):
            L.rank_ap(torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda"), p)
    # ... which the module answers with its plain path
    m = L.SupAP(offset=1.44)
    s = torch.rand(1, C.COLS_MAX + 1, device="cuda")
    t = (torch.rand(1, C.COLS_MAX + 1, device="cuda") < 0.01).float()
    t[0, 0] = 1
    assert torch.isfinite(m(s, t)) and m(s, t).is_cuda


def test_call_on_a_side_stream():
    case = next(c for c in C.CASES if c.name == "batch96" and c.kind == "sup" and c.form == "quick")
    x = C.inputs(case)
    s, t = x.scores.cuda(), x.target.cuda()
    want = L.rank_ap(s, t, C.params_of(x))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = L.rank_ap(s, t, C.params_of(x))
    side.synchronize()
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))


@pytest.mark.parametrize("kind", ["smooth", "sup", "sup_auto"])
@pytest.mark.parametrize("form", ["quick", "general"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_function_agrees_with_the_plain_path(kind, form, dtype, monkeypatch):
    """Value and gradient through a non-unit grad_output, against the plain path on the widened values: 3 * (1 - mAP), and
    the per-row AP weighted row by row."""
    case = next(c for c in C.CASES if c.name == "batch96" and c.kind == "sup_auto" and c.form == form)._replace(kind=kind)
    x = C.inputs(case)
    general = form == "general"
    tgt = x.target.cuda()
    rounded = x.scores.to(dtype)
    assert C.near_delta(rounded.float(), x.target) == 0
    calls = []
    fused = L.rank_ap
    monkeypatch.setattr(L, "rank_ap", lambda *a, **k: calls.append(k.get("want_grad")) or fused(*a, **k))
    weights = torch.linspace(0.5, 2.0, case.B, device="cuda")
    for return_type, reduce in (("1-mAP", lambda v: 3.0 * v), ("AP", lambda v: (weights * v).sum())):
        m = C.module_of(case, return_type)
        assert m.fused and m.check_labels
        calls.clear()
        s = rounded.cuda().requires_grad_(True)
        val = m(s, tgt, force_general=general)
        reduce(val).backward()
        assert calls == [True] and val.dtype == torch.float32 and s.grad.dtype == dtype
        m.fused = False
        wide = rounded.cuda().float().requires_grad_(True)
        ref = m(wide, tgt, force_general=general)
        reduce(ref).backward()
        assert calls == [True]                                   # the plain path made no library call
        ev = max(C.scalar_err(a, b) for a, b in zip(val.reshape(-1), ref.detach().double().reshape(-1)))
        if dtype == torch.float32:
            ge = C.grad_err(s.grad, wide.grad.double())
            print(f"{kind} {form} {return_type} {dtype}: value {ev:.2e} grad {ge:.2e}")
            assert ev <= C.TOL and ge <= C.TOL
        else:
            slack = C.bf16_grad_slack(s.grad, wide.grad)
            print(f"{kind} {form} {return_type} {dtype}: value {ev:.2e} grad, worst element over its allowance {slack:.2e}")
            assert ev <= C.TOL and slack <= 0.0
        m.fused = True
        with torch.no_grad():
            quiet = m(s, tgt, force_general=general)
        assert calls == [True, False] and torch.equal(_bits(quiet), _bits(val))
        flat = m(s.detach(), tgt, force_general=general)          # scores that need no gradient: the null pointer too
        assert calls == [True, False, False] and torch.equal(_bits(flat), _bits(val))
    # what the fused path does not take goes to the plain path, on the same device, without a library call
    calls.clear()
    s = rounded.cuda().float()
    assert m(s.double(), tgt, force_general=general).dtype == torch.float64
    assert m(s, 2.0 * tgt, force_general=general).is_cuda
    empty = tgt.clone()
    empty[5] = 0
    assert torch.isnan(m(s, empty, force_general=general)[5])     # the reference's 0 / 0
    if not general:
        holed = tgt.clone()
        holed[5, 5] = 0
        m(s, holed)
    assert calls == []
    m.check_labels = False
    m(s, tgt, force_general=general)
    assert calls == [False]
    assert L.HeavisideAP()(s, tgt).is_cuda and calls == [False]


def test_train_steps_on_the_baseline_under_sup_ap():
    from wvhash.engine import train_step
    from wvhash.models import DINOHashBaseline
    torch.manual_seed(0)
    net = DINOHashBaseline(binary_config={"nbits": 64}, frozen=True, backbone=SB.TinyBackbone(seed=2)).cuda().train()
    crit = L.SupAP(tau=0.01, rho=100.0, offset=1.44, delta=0.05)
    assert crit.fused and not hasattr(crit, "takes_embeddings")
    g = torch.Generator().manual_seed(1)
    images = torch.rand(48, 3, 16, 16, generator=g)
    labels = C.multi_hot(48, 5)
    # raw logits make scores of tens: most sigmoids are saturated and the linear part (slope rho) carries the descent.  fp32
    # scores: under bf16 autocast they sit on a grid of 1 / 8 and coarser, and six steps move the ranks by less than that
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=0.001)
    seen = [train_step(net, images, labels, [(crit, 1.0)], [opt], autocast_dtype=None)["SupAP"] for _ in range(6)]
    print("SupAP (1 - mAP) over six steps:", seen)
    assert all(v == v for v in seen) and seen[-1] < seen[0]
