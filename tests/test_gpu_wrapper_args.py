"""The Hamming wrappers (wvhash/engine/hamming.py) on the GPU with every tensor form of tests/wrapper_arg_cases.py: each
accepted form (strided rows, column slices, offset views, column-major views, int64 index lists, list prefixes) gives exactly
the canonical call's outputs -- the same kernel on the same bytes after the gate's copy --, the canonical call gives the
oracle's, and the host twin (engine/hamming_host.py) gives the same for the same form.  Every refused form raises ValueError
and leaves the caller's buffers as they were; tests/test_wrapper_args.py proves on the host that none of them reaches an
entry point, which is why they may be tried here at all."""
import pytest
import torch

import ndcg_cases
import wrapper_arg_cases as C
from oracle import ranking
from wvhash import _lib
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming as H
from wvhash.engine import hamming_host as HH

pytestmark = pytest.mark.gpu
AP_TOL = 1e-6                    # tests/test_gpu_ranking.py's: fp32 AP against the oracle's
FILL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: -7, torch.uint8: 0xA5}


def _setup(run):
    case, cfg, k = run
    w = C.world(*cfg)
    host = {name: t.clone() for name, t in case.canon(w, k).items()}
    dev = {name: t.cuda() for name, t in host.items()}
    if "workspace" in host:                                    # the table's workspace must be the one the call uses
        need = _lib.load().wv_hamming_topk_workspace_bytes(w.Q, w.N, w.qp.shape[1], k)
        assert need <= C.WORKSPACE_BYTES
    return case, w, k, host, dev


def _check(out, want, what):
    assert len(out) == len(want), what
    for o, e in zip(out, want):
        assert (o is None) == (e is None), what
        if e is None:
            continue
        exp, mode = e
        assert tuple(o.shape) == tuple(exp.shape), what
        if mode == C.EXACT:
            assert o.dtype == exp.dtype and torch.equal(o.cpu(), exp), what
        elif mode == C.AP:
            assert o.dtype == torch.float32 and float((o.cpu().double() - exp).abs().max()) <= AP_TOL, what
        elif mode == C.DCG:
            tol = torch.tensor([ndcg_cases.sum_tol(kk) for kk in C.KS], dtype=torch.float64)
            assert o.dtype == torch.float64 and bool(((o.cpu() - exp).abs() <= tol * exp.abs()).all()), what


def _same(out, ref, what):
    """every output equal bit for bit (floats compared as their bits' values: no NaN is expected anywhere)"""
    assert len(out) == len(ref), what
    for o, c in zip(out, ref):
        assert (o is None) == (c is None), what
        if o is not None:
            assert o.dtype == c.dtype and o.shape == c.shape and torch.equal(o.cpu(), c.cpu()), what
            assert not o.is_floating_point() or not bool(torch.isnan(o).any()), what


@pytest.mark.parametrize("run", C.runs(), ids=C.run_id)
def test_accepted_forms_equal_the_canonical_call_the_oracle_and_the_host_twin(run):
    case, w, k, host, dev = _setup(run)
    x = case.prepare(H, dev)
    canon = case.call(H, w, k, dev, x)
    _check(canon, case.want(w, k), (case.name, "canonical"))
    if case.twin:
        xh = case.prepare(HH, host)
        _same(canon, case.call(HH, w, k, host, xh), (case.name, "canonical", "twin"))
    for arg in case.args:
        for form in C.accepted_forms(arg):
            what = (case.name, arg.name, form)
            got = case.call(H, w, k, dict(dev, **{arg.name: C.make_accepted(form, arg, dev[arg.name])}), x)
            _same(got, canon, what)
            if case.twin:                                      # both backends see the same form
                twin = case.call(HH, w, k, dict(host, **{arg.name: C.make_accepted(form, arg, host[arg.name])}), xh)
                _same(got, twin, what + ("twin",))


@pytest.mark.parametrize("run", C.runs(), ids=C.run_id)
def test_refused_forms_raise_and_leave_the_callers_buffers_alone(run):
    case, w, k, host, dev = _setup(run)
    x = case.prepare(H, dev)
    written = [arg.name for arg in case.args if arg.kind == C.WRITTEN]
    for name in written:
        dev[name].fill_(FILL[dev[name].dtype])
    for arg in case.args:
        for form in C.refused_forms(arg):
            given = C.make_refused(form, arg, dev[arg.name], lambda t: t.cpu())
            before = given.clone()
            with pytest.raises(ValueError, match=case.name.replace("_want_cum", "")):
                case.call(H, w, k, dict(dev, **{arg.name: given}), x)
            assert torch.equal(given, before), (case.name, arg.name, form)
            for name in written:
                assert bool((dev[name] == FILL[dev[name].dtype]).all()), (case.name, arg.name, form, name)


def test_map_at_k_takes_the_int64_lists_get_knn_hands_out():
    """The bug this file is named for: map_at_k(hamming_topk(...)[0].long(), ...) read the int64 lists as int32 pairs, so
    every second entry was row 0 and the AP simply wrong.  Now: the AP of the int32 lists, the oracle's, on both backends."""
    w = C.world(3000, 64, 38)
    k = 100
    qp, rp, qlp, rlp = w.qp.cuda(), w.rp.cuda(), w.qlp.cuda(), w.rlp.cuda()
    idx = H.hamming_topk(qp, rp, w.nbits, k)[0]
    assert torch.equal(idx.cpu(), w.order[:, :k])
    ap32, nrel32 = H.map_at_k(idx, qlp, rlp)
    ap64, nrel64 = H.map_at_k(idx.long(), qlp, rlp)
    assert torch.equal(ap64, ap32) and torch.equal(nrel64, nrel32) and int(nrel64.max()) > 0
    want_ap, want_nrel = w.ap(k)
    assert float((ap64.cpu().double() - want_ap).abs().max()) <= AP_TOL and torch.equal(nrel64.cpu(), want_nrel)
    ap_h, nrel_h = HH.map_at_k(idx.cpu().long(), w.qlp, w.rlp)
    assert torch.equal(ap64.cpu(), ap_h) and torch.equal(nrel64.cpu(), nrel_h)
    want = ranking.calculate_maphashing(w.q, w.ql, w.r, w.rl, k, stable=True)
    assert abs(float(ap64.double().mean()) - want) < AP_TOL
    for device in (None, "cpu"):
        calc = CustomCalculator(k=k, device=device, distance_metric="hamming", with_faiss=False)
        assert abs(calc.calculate_maphashing(w.q, w.ql, w.r, w.rl, k) - want) < AP_TOL, device
