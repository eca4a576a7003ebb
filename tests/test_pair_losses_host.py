"""SCHLoss and HashNetAdapter (wvhash/losses.py) without a GPU: the plain PyTorch path and the host twin wv_pair_loss_cpu
against the reference-made goldens (tests/golden/pair_losses_golden.npz, make_golden_pair_losses.py) and against the float64
restatement of tests/pair_loss_cases.py; the modules' surface (attributes, state_dict, the step() schedule, the fixed 0.1
alpha, the label rule); the entry points' argument gate; and train_step stepping a criterion that has step() but no
optimizer, over real gloo ranks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pair_loss_cases as C
from wvhash import _lib
from wvhash import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pair_losses_golden.npz"))


# name -> (loss, alpha, beta, apply_tanh, scale, labels): what make_golden_pair_losses.py ran the reference with
GOLDEN_CASES = {
    "sch_tanh_b1": ("sch", 1.0, 1.0, True, 1, "dense"),
    "sch_pre_b01": ("sch", 1.0, 0.1, False, 1, "dense"),
    "sch_a01": ("sch", 0.1, 0.1, True, 1, "tags14"),
    "hashnet_s1": ("hashnet", 0.1, 0.0, True, 1, "dense"),
    "hashnet_s3": ("hashnet", 0.1, 0.0, True, 3, "dense"),
}
GOLDEN_SHAPES = [(96, 64, 38), (64, 16, 20), (33, 64, 24), (257, 128, 80)]


def _module(loss, D, alpha, beta, apply_tanh, scale):
    if loss == "sch":
        return L.SCHLoss(n_bits=D, alpha=alpha, beta=beta, apply_tanh=apply_tanh)
    m = L.HashNetAdapter(embedding_size=D, alpha=alpha)
    m.criterion.scale = scale
    return m


def _golden_inputs(golden, shape, name):
    B, D, Cn = shape
    loss, alpha, beta, apply_tanh, scale, which = GOLDEN_CASES[name]
    tag = f"{B}x{D}x{Cn}"
    e = torch.from_numpy(golden[f"{tag}/logits" if apply_tanh else f"{tag}/pre"])
    lab = torch.from_numpy(golden[f"{tag}/labels_{which}"]).float()
    return e, lab, float(golden[f"{tag}/{name}/loss"][0]), torch.from_numpy(golden[f"{tag}/{name}/grad"])


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_plain_path_twin_and_restatement_meet_the_reference_made_goldens(golden, shape, name):
    assert list(golden["shapes"].tolist()) == [list(s) for s in GOLDEN_SHAPES] and sorted(golden["cases"]) == sorted(GOLDEN_CASES)
    loss, alpha, beta, apply_tanh, scale, _ = GOLDEN_CASES[name]
    D = shape[1]
    e, lab, want, want_grad = _golden_inputs(golden, shape, name)
    # the plain path, fp32 on the CPU, by autograd
    x = e.clone().requires_grad_(True)
    got = _module(loss, D, alpha, beta, apply_tanh, scale)(x, lab)
    got.backward()
    ev, eg = C.scalar_err(got, want), C.grad_err(x.grad, want_grad)
    print(f"plain: loss {ev:.2e} grad {eg:.2e}")
    assert ev <= C.TOL and eg <= C.TOL
    # the host twin
    params = L.pair_loss_params(loss, apply_tanh, scale, D, alpha, beta)
    out, grad = L.pair_loss_host(e, C.pack_bits(lab), params)
    ev, eg = C.scalar_err(out[0], want), C.grad_err(grad, want_grad)
    print(f"twin: loss {ev:.2e} grad {eg:.2e}")
    assert ev <= C.TOL and eg <= C.TOL
    assert abs(float(out[1]) + float(out[2]) - float(out[0])) <= 1e-6 * abs(float(out[0]))
    # the float64 restatement the GPU tests use as their reference describes the same function
    r_out, r_grad = C.restate64(loss, e, lab, apply_tanh, scale, D, alpha, beta)
    assert C.scalar_err(want, r_out[0]) <= C.TOL and C.grad_err(want_grad, r_grad) <= C.TOL


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_twin_equals_plain_path_and_restatement(case):
    """On the shape list of the kernel: the twin and the plain path (fp32) within TOL of the float64 restatement, and the
    plain path run in float64 equal to the restatement to 1e-12."""
    x = C.inputs(case)
    ref_out, ref_grad = C.reference(case)
    out, grad = L.pair_loss_host(x.e, x.packed, C.params_of(x))
    C.check(out, grad, ref_out, ref_grad, "twin")
    assert torch.equal(L.pair_loss_host(x.e, x.packed, C.params_of(x), want_grad=False)[0], out)
    for dtype, tol in ((torch.float32, C.TOL), (torch.float64, 1e-12)):
        e = x.e.clone().to(dtype).requires_grad_(True)
        m = _module(x.loss, case.D, x.alpha, x.beta, x.apply_tanh, x.pre_scale)
        val = m(e, x.labels)
        val.backward()
        assert val.dtype == dtype
        assert C.scalar_err(val, ref_out[0]) <= tol and C.grad_err(e.grad, ref_grad) <= tol, dtype


def test_zero_norm_part_has_zero_gradient_and_no_nan():
    case = next(c for c in C.CASES if c.labels == "onehot")
    x = C.inputs(case)
    ref_out, ref_grad = C.reference(case)
    assert float(ref_out[2]) == 0.0 and float(ref_out[1]) > 0.0
    out, grad = L.pair_loss_host(x.e, x.packed, C.params_of(x))
    assert float(out[2]) == 0.0 and torch.isfinite(grad).all()
    e = x.e.clone().requires_grad_(True)
    L.SCHLoss(n_bits=case.D, alpha=x.alpha, beta=x.beta)(e, x.labels).backward()
    assert torch.isfinite(e.grad).all() and C.grad_err(e.grad, ref_grad) <= C.TOL
    # every pair disjoint and nothing closer than k / 2: both parts can vanish -- all zeros, never NaN
    out, grad = L.pair_loss_host(torch.zeros(4, 8), torch.zeros((4, 1), dtype=torch.int64), L.pair_loss_params("sch", False, 1.0, 8, 1.0, 1.0))
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()


def test_module_surface():
    s = L.SCHLoss()
    assert (s.n_bits, s.alpha, s.beta, s.apply_tanh, s.takes_embeddings) == (64, 0.1, 0.1, False, True)
    assert isinstance(s.max_func, torch.nn.ReLU) and list(s.parameters()) == [] and len(s.state_dict()) == 0
    assert (s.fused, s.check_labels) == (True, True)
    s = L.SCHLoss(32, 1, 1, True, "ignored", more="ignored")
    assert (s.n_bits, s.alpha, s.beta, s.apply_tanh) == (32, 1, 1, True)

    h = L.HashNetAdapter()
    assert h.takes_embeddings and isinstance(h.criterion, L.HashNetLoss) and h.criterion.scale == 1
    assert (h.global_batch_step, h.step_continuation, h.batches_per_epoch) == (0, 20, 49)
    assert list(h.parameters()) == [] and len(h.state_dict()) == 0          # the step counter does not travel: scale restarts at 1
    h = L.HashNetAdapter(embedding_size=16, alpha=0.7, step_continuation=2, batches_per_epoch=3, extra=1)
    scales = []
    for _ in range(13):
        h.step()
        scales.append(h.criterion.scale)
    assert h.global_batch_step == 13 and scales == [1] * 5 + [2] * 6 + [3] * 2    # (step // 3) // 2 + 1
    fresh = L.HashNetAdapter(embedding_size=16, step_continuation=2, batches_per_epoch=3)
    fresh.load_state_dict(h.state_dict())
    assert fresh.global_batch_step == 0 and fresh.criterion.scale == 1
    h.fused = False
    assert h.criterion.fused is False and h.fused is False
    h.check_labels = False
    assert h.criterion.check_labels is False

    # the adapter passes alpha = 0.1 whatever the constructor got
    g = torch.Generator().manual_seed(0)
    e, lab = torch.randn(9, 16, generator=g), (torch.rand(9, 6, generator=g) < 0.3).float()
    a, b = L.HashNetAdapter(embedding_size=16, alpha=0.7), L.HashNetAdapter(embedding_size=16, alpha=0.1)
    assert torch.equal(a(e, lab), b(e, lab))
    assert torch.equal(a(e, lab), a.criterion(u=e, y=lab, ind=None, config={"alpha": 0.1}))
    assert not torch.equal(a(e, lab), a.criterion(u=e, y=lab, ind=None, config={"alpha": 0.7}))


def test_class_id_labels_are_refused():
    e = torch.randn(5, 8)
    for m in (L.SCHLoss(n_bits=8), L.HashNetAdapter(embedding_size=8)):
        with pytest.raises(ValueError, match="2-D multi-hot"):
            m(e, torch.arange(5))


def test_plain_path_takes_what_the_fused_path_does_not():
    """CPU tensors, fp64, bf16 on the host (widened: an fp32 loss), labels that are not 0/1 -- never an error, never a device
    change; and autocast does not reach into the loss."""
    g = torch.Generator().manual_seed(3)
    e, lab = torch.randn(12, 16, generator=g), (torch.rand(12, 7, generator=g) < 0.3).float()
    for m in (L.SCHLoss(n_bits=16, apply_tanh=True), L.HashNetAdapter(embedding_size=16)):
        want = m(e, lab)
        assert want.device.type == "cpu" and want.dtype == torch.float32
        eb = e.bfloat16().requires_grad_(True)
        got = m(eb, lab)
        got.backward()
        assert got.dtype == torch.float32 and eb.grad.dtype == torch.bfloat16
        assert torch.equal(got, m(e.bfloat16().float(), lab))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert torch.equal(m(e, lab), want)
        assert torch.isfinite(m(e, 2.5 * lab))                  # weighted labels: the reference's real-valued relation
        assert m(e.double(), lab).dtype == torch.float64


def _gate(gpu, e, labels, lwords, B, D, params, out, ws=None, ws_bytes=0):
    lib = _lib.load()
    if gpu:
        return lib.wv_pair_loss(e, labels, lwords, B, D, params, out, None, ws, ws_bytes, None)
    return lib.wv_pair_loss_cpu(e, labels, lwords, B, D, params, out, None)


@pytest.mark.parametrize("gpu", [False, True], ids=["twin", "kernel"])
def test_argument_gate_answers_before_any_pointer_is_read(gpu):
    lib = _lib.load()
    one = ctypes.c_void_p(16)                     # never dereferenced: every call below is refused first
    ok = ctypes.byref(L.pair_loss_params("sch"))
    big = 1 << 40
    name = b"pair_loss:" if gpu else b"pair_loss_cpu:"

    def call(e=one, labels=one, lwords=1, B=8, D=16, params=ok, out=one, ws=one, ws_bytes=big):
        return _gate(gpu, e, labels, lwords, B, D, params, out, ws, ws_bytes)

    for kw, word in ((dict(e=None), b"e is null"), (dict(labels=None), b"labels is null"), (dict(params=None), b"params is null"),
                     (dict(out=None), b"out is null"), (dict(B=0), b"B=0"), (dict(D=0), b"D=0"), (dict(lwords=0), b"lwords=0"),
                     (dict(lwords=3), b"lwords=3"), (dict(params=ctypes.byref(L.pair_loss_params(2))), b"kind=2"),
                     (dict(params=ctypes.byref(L.pair_loss_params("hashnet", True, 0.0))), b"pre_scale=0"),
                     (dict(params=ctypes.byref(L.pair_loss_params("hashnet", True, -1.0))), b"pre_scale=-1")):
        assert call(**kw) == -22, kw
        msg = lib.wv_last_error()
        assert msg.startswith(name) and word in msg, (kw, msg)
    assert call(B=2049) == -95 and b"WV_PAIR_LOSS_ROWS_MAX=2048" in lib.wv_last_error()
    assert call(D=513) == -95 and b"D=513" in lib.wv_last_error()
    if gpu:
        need = lib.wv_pair_loss_workspace_bytes(8, 16)
        assert need == 2 * 8 * 16 * 4 + 32 and lib.wv_pair_loss_workspace_bytes(9, 16) == 2 * 9 * 16 * 4 + 2 * 32
        assert lib.wv_pair_loss_workspace_bytes(0, 16) == 0
        assert call(ws=None) == -22 and b"workspace is null" in lib.wv_last_error()
        assert call(ws_bytes=need - 1) == -22 and b"workspace" in lib.wv_last_error()


def test_wrapper_gate():
    e, lp = torch.randn(6, 8), torch.zeros((6, 1), dtype=torch.int64)
    p = L.pair_loss_params("sch", nbits=8)
    with pytest.raises(ValueError, match="pair_loss_host: e: expected dtype torch.float32"):
        L.pair_loss_host(e.double(), lp, p)
    with pytest.raises(ValueError, match="pair_loss_host: labels_packed: expected shape"):
        L.pair_loss_host(e, lp[:5], p)
    with pytest.raises(ValueError, match="pair_loss_host: labels_packed: expected dtype torch.int64"):
        L.pair_loss_host(e, lp.int(), p)
    with pytest.raises(ValueError, match="pair_loss: e: expected a tensor on a cuda device"):
        L.pair_loss(e, lp, p)
    with pytest.raises(ValueError, match="params: expected a PairLossParams"):
        L.pair_loss_host(e, lp, {"kind": 0})
    with pytest.raises(_lib.WvhashUnsupported, match="D=513"):
        L.pair_loss_host(torch.zeros(2, 513), lp[:2], p)
    with pytest.raises(ValueError, match="lwords=3"):
        L.pair_loss_host(e, torch.zeros((6, 3), dtype=torch.int64), p)
    out, grad = L.pair_loss_host(e.t().contiguous().t(), lp, p)           # a strided view is copied, not misread
    assert torch.equal(out, L.pair_loss_host(e, lp, p)[0]) and grad.shape == e.shape
    half = e.bfloat16()
    assert torch.equal(L.pair_loss_host(half, lp, p)[0], L.pair_loss_host(half.float(), lp, p)[0])


@pytest.mark.parametrize("kind", ["sch_tanh", "hashnet_s3"])
def test_fused_function_over_the_host_twin(kind):
    """The autograd Function of the modules' fused path, run over pair_loss_host: value and gradient through a non-unit
    grad_output (3 * loss) against the plain path on the same fp32 input; a bf16 input gets a bf16 gradient; with
    want=False nothing is saved and the value has the same bits."""
    case = next(c for c in C.CASES if c.B == 33 and c.D == 64 and c.kind == kind)
    x = C.inputs(case)
    params = C.params_of(x)
    e = x.e.clone().requires_grad_(True)
    val = L._FusedLoss.apply(L.pair_loss_host, 0, e, x.packed, params, True)
    (3.0 * val).backward()
    wide = x.e.clone().requires_grad_(True)
    ref = _module(x.loss, case.D, x.alpha, x.beta, x.apply_tanh, x.pre_scale)(wide, x.labels)
    (3.0 * ref).backward()
    ev, eg = C.scalar_err(val, ref.detach().double()), C.grad_err(e.grad, wide.grad.double())
    print(f"{kind}: loss {ev:.2e} grad {eg:.2e}")
    assert val.shape == () and val.dtype == torch.float32 and e.grad.dtype == torch.float32
    assert ev <= C.TOL and eg <= C.TOL
    eb = x.e.bfloat16().requires_grad_(True)
    L._FusedLoss.apply(L.pair_loss_host, 0, eb, x.packed, params, True).backward()
    assert eb.grad.dtype == torch.bfloat16 and eb.grad.shape == eb.shape
    quiet = L._FusedLoss.apply(L.pair_loss_host, 0, e, x.packed, params, False)
    assert quiet.grad_fn.saved_tensors == ()
    assert torch.equal(quiet.detach().view(torch.int32), val.detach().view(torch.int32))


# ------------------------------------------------------------------------------------------------ train_step, gloo
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "image-retrieval-wavelet_amd"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from wvhash.engine import make_averager, train_step
    from wvhash.losses import HashNetAdapter
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 8))
    crit = HashNetAdapter(embedding_size=8, step_continuation=1, batches_per_epoch=2)
    criteria = [(crit, 1.0)]
    g = torch.Generator().manual_seed(7 + rank)
    x, y = torch.randn(6, 3, 2, 2, generator=g), (torch.rand(6, 5, generator=g) < 0.4).float()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    avg = make_averager(net, criteria)
    seen = []
    for _ in range(5):
        logs = train_step(net, x, y, criteria, [opt], averager=avg, autocast_dtype=None)
        seen.append((crit.global_batch_step, crit.criterion.scale, logs["HashNetAdapter"]))
    torch.save({"seen": seen, "w": net[1].weight.detach().clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_train_step_steps_a_criterion_without_an_optimizer(tmp_path):
    port = 31600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(2)]
    for r in range(2):
        steps = [(s, sc) for s, sc, _ in got[r]["seen"]]
        assert steps == [(1, 1), (2, 2), (3, 2), (4, 3), (5, 3)], steps       # once per train_step; (step // 2) // 1 + 1
        assert all(np.isfinite(v) for _, _, v in got[r]["seen"])
    assert torch.equal(got[0]["w"], got[1]["w"])
