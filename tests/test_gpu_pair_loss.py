"""wv_pair_loss on the GPU: the kernel's out / grad against the float64 restatement and the host twin on every case of
tests/pair_loss_cases.py (row-block and column-tile edges, one and two label words, D = 1 ... 512, all-identical and
all-empty labels, a part that is exactly zero), the row limit, run-to-run bits, a side stream, grad = NULL, the fused
autograd Function against the plain path (fp32 and bf16 inputs, a non-unit grad_output, no_grad), and one train_step on
DINOHashBaseline under SCHLoss."""
import pytest
import torch

import pair_loss_cases as C
import single_band_cases as SB
from wvhash import losses as L

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(x, want_grad=True):
    return L.pair_loss(x.e.cuda(), x.packed.cuda(), C.params_of(x), want_grad=want_grad)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernel_against_float64_and_the_twin(case):
    x = C.inputs(case)
    ref_out, ref_grad = C.reference(case)
    out, grad = _run(x)
    assert out.dtype == torch.float32 and grad.dtype == torch.float32 and grad.shape == x.e.shape
    C.check(out.cpu(), grad.cpu(), ref_out, ref_grad, "kernel vs float64")
    t_out, t_grad = L.pair_loss_host(x.e, x.packed, C.params_of(x))
    C.check(out.cpu(), grad.cpu(), t_out.double(), t_grad.double(), "kernel vs twin")
    # the same call again: the same bits; without the gradient: the same out bits
    out2, grad2 = _run(x)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(grad), _bits(grad2))
    out3, none = _run(x, want_grad=False)
    assert none is None and torch.equal(_bits(out), _bits(out3))


def test_zero_part_gives_zero_gradient_and_no_nan():
    for case in (c for c in C.CASES if c.labels in ("onehot", "empty") and c.kind.startswith("sch")):
        ref_out, _ = C.reference(case)
        out, grad = _run(C.inputs(case))
        assert float(ref_out[2]) == 0.0 and float(out[2]) == 0.0 and torch.isfinite(grad).all() and torch.isfinite(out).all()
    z = L.pair_loss(torch.zeros(4, 8, device="cuda"), torch.zeros((4, 1), dtype=torch.int64, device="cuda"),
                    L.pair_loss_params("sch", False, 1.0, 8, 1.0, 1.0))
    assert float(z[0].abs().max()) == 0.0 and float(z[1].abs().max()) == 0.0          # both norms 0: all zeros


def test_row_limit_2048():
    case = C.BIG_CASE
    x = C.inputs(case)
    ref_out, ref_grad = C.reference(case)
    out, grad = _run(x)
    C.check(out.cpu(), grad.cpu(), ref_out, ref_grad, "kernel vs float64, 2048 x 64")
    out2, grad2 = _run(x)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(grad), _bits(grad2))
    with pytest.raises(Exception, match="WV_PAIR_LOSS_ROWS_MAX"):
        L.pair_loss(torch.zeros(2049, 4, device="cuda"), torch.zeros((2049, 1), dtype=torch.int64, device="cuda"), C.params_of(x))


def test_call_on_a_side_stream():
    case = next(c for c in C.CASES if c.B == 96 and c.kind == "hashnet_s3")
    x = C.inputs(case)
    e, lp = x.e.cuda(), x.packed.cuda()
    want = L.pair_loss(e, lp, C.params_of(x))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = L.pair_loss(e, lp, C.params_of(x))
    side.synchronize()
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))


def _module(x, D):
    if x.loss == "sch":
        return L.SCHLoss(n_bits=D, alpha=x.alpha, beta=x.beta, apply_tanh=x.apply_tanh)
    m = L.HashNetAdapter(embedding_size=D)
    m.criterion.scale = x.pre_scale
    return m


@pytest.mark.parametrize("kind", sorted(C.KINDS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_function_agrees_with_the_plain_path(kind, dtype, monkeypatch):
    """Value and gradient through a non-unit grad_output (3 * loss), against the plain path on the widened values."""
    case = next(c for c in C.CASES if c.B == 33 and c.D == 64 and c.kind == kind)
    x = C.inputs(case)
    m = _module(x, case.D)
    m.fused = True                                               # whatever the module's default is
    lab = x.labels.cuda()
    calls = []
    fused = L.pair_loss
    monkeypatch.setattr(L, "pair_loss", lambda *a, **k: calls.append(k.get("want_grad")) or fused(*a, **k))
    e = x.e.cuda().to(dtype).requires_grad_(True)
    val = m(e, lab)
    (3.0 * val).backward()
    assert calls == [True] and val.dtype == torch.float32 and e.grad.dtype == dtype
    m.fused = False
    wide = x.e.cuda().to(dtype).float().requires_grad_(True)
    ref = m(wide, lab)
    (3.0 * ref).backward()
    assert calls == [True]                                       # the plain path made no library call
    ev = C.scalar_err(val, ref.detach().double())
    if dtype == torch.float32:
        ge = C.grad_err(e.grad, wide.grad.double())
        print(f"{kind} {dtype}: loss {ev:.2e} grad {ge:.2e}")
        assert ev <= C.TOL and ge <= C.TOL
    else:
        slack = C.bf16_grad_slack(e.grad, wide.grad)
        print(f"{kind} {dtype}: loss {ev:.2e} grad, worst element over its allowance {slack:.2e}")
        assert ev <= C.TOL and slack <= 0.0
    m.fused = True
    with torch.no_grad():
        quiet = m(e, lab)
    assert calls == [True, False] and torch.equal(_bits(quiet), _bits(val))
    # labels that are not 0/1 and fp64 embeddings take the plain path, on the same device
    calls.clear()
    assert m(e.detach().double(), lab).is_cuda and m(e.detach().float(), 2.0 * lab).is_cuda and calls == []
    m.check_labels = False
    m(e.detach().float(), lab)
    assert calls == [False]


def test_train_step_on_the_baseline_under_sch_loss():
    from wvhash.engine import train_step
    from wvhash.models import DINOHashBaseline
    torch.manual_seed(0)
    net = DINOHashBaseline(binary_config={"nbits": 64}, frozen=True, backbone=SB.TinyBackbone(seed=2)).cuda().train()
    crit = L.SCHLoss(n_bits=64, alpha=1, beta=1, apply_tanh=True)
    crit.fused = True
    g = torch.Generator().manual_seed(1)
    images = torch.rand(48, 3, 16, 16, generator=g)
    labels = C.make_labels(48, 38, "dense", 5)
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=0.005)
    seen = [train_step(net, images, labels, [(crit, 1.0)], [opt])["SCHLoss"] for _ in range(6)]
    print("SCHLoss over six steps:", seen)
    assert all(v == v for v in seen) and seen[-1] < seen[0]
