"""wv_hamming_radius_hist (k_rank_radius, csrc/rank2.hip) on the GPU: both tables equal a brute-force expectation AND the
host twin exactly at the smallest shapes where the kernel can go wrong, and the metrics built on them reproduce the values the
REFERENCE's own pr_curve / get_precision_recall_by_Hamming_Radius produced (tests/golden/radius_golden.npz)."""
import os

import numpy as np
import pytest
import torch

import radius_cases as rc
from wvhash import _lib
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming as H
from wvhash.engine import hamming_host as HH
from wvhash.engine import radius_metrics as RM
from wvhash.engine.accuracy_calculator import RankCache

pytestmark = pytest.mark.gpu

# threads without items, a ragged last thread, both ends of the register buckets (C = 16 | 17, 128), one and two code words,
# a width that is no multiple of 64, one and two label words, one / few / more queries than a wave
NS = [1, 255, 257, 4096, 4097, 32767, 32768]
NBITS = [16, 48, 64, 128]
SHAPES = [(N, nbits, (12, 80)[(i + j) % 2], (1, 5, 67)[(i + j) % 3]) for i, N in enumerate(NS) for j, nbits in enumerate(NBITS)]


def _gpu_tables(q, r, ql, rl):
    nbits = q.shape[1]
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    return H.hamming_radius_hist(qp, H.PreparedDB(rp, nbits), H.PreparedLabels(rlp), qlp, nbits)


def _twin_tables(q, r, ql, rl):
    return HH.hamming_radius_hist(HH.pack_codes(q), HH.pack_codes(r), HH.pack_labels(rl), HH.pack_labels(ql), q.shape[1])


def _check(q, r, ql, rl):
    got = _gpu_tables(q, r, ql, rl)
    assert got is not None and got[0].dtype == torch.int32 and tuple(got[0].shape) == tuple(got[1].shape) == (q.shape[0], q.shape[1] + 2)
    want = rc.brute_tables(q.cuda(), r.cuda(), ql.cuda(), rl.cuda())
    twin = _twin_tables(q, r, ql, rl)
    for i in range(2):
        assert torch.equal(got[i], want[i]), ("kernel != brute force", i)
        assert torch.equal(got[i].cpu(), twin[i]), ("kernel != host twin", i)
    return got


@pytest.mark.parametrize("N,nbits,classes,Q", SHAPES)
def test_tables_equal_brute_force_and_the_twin(N, nbits, classes, Q):
    q, r, ql, rl = rc.make_inputs(Q, N, nbits, classes, seed=N + nbits)
    cum, cumrel = _check(q, r, ql, rl)
    assert bool((cum[:, -1] == N).all())
    assert bool((cumrel[0] == 0).all())                                            # query 0: zero label words
    if N >= 8:
        assert bool((cum[:min(Q, 4), 1] >= 2).all())                               # duplicate rows at distance 0
        if Q > 1:
            assert 1 <= int(cumrel[1, 1]) < int(cum[1, 1])                         # ... one relevant, one not
    if classes > 64 and Q > 1 and N >= 255:
        assert int(cumrel[Q - 1, -1]) > 0                                          # classes of the second label word only


@pytest.mark.parametrize("nbits,classes", [(64, 12), (128, 80)])
def test_every_row_in_one_bin(nbits, classes):
    """A database of identical codes, all of them relevant to some queries: one bin takes all 32,768 rows, every shared
    16-bit half cell its maximum (16 threads x 128 items)."""
    q, r, ql, rl = rc.make_inputs(5, 32768, nbits, classes, seed=7, identical=True)
    rl[:, 3] = 1.0
    ql[1, 3] = 1.0
    ql[2] = 0
    ql[2, 3] = 1.0
    cum, cumrel = _check(q, r, ql, rl)
    assert int(cum[2, 1]) == 32768 and int(cumrel[2, 1]) == 32768 and int(cumrel[0, -1]) == 0   # query 2's code is the rows'


def test_virtual_shards_add_up():
    q, r, ql, rl = rc.make_inputs(9, 40000, 64, 12, seed=11)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    db, lab = H.PreparedDB(rp, 64), H.PreparedLabels(H.pack_labels(rl.cuda()))
    assert db.parts and len(db.parts) == 2 and lab.parts
    got = H.hamming_radius_hist(qp, db, lab, H.pack_labels(ql.cuda()), 64)
    want = rc.brute_tables(q.cuda(), r.cuda(), ql.cuda(), rl.cuda())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_shapes_outside_the_kernel_are_refused():
    lib = _lib.require_gpu()
    q, r, ql, rl = rc.make_inputs(3, 32769, 64, 12, seed=5)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    db = H.PreparedDB(rp, 64, _virtual=False)
    small = H.PreparedLabels(rlp[:100].contiguous())
    out = torch.zeros((2, 3, 66), dtype=torch.int32, device="cuda")
    rcode = lib.wv_hamming_radius_hist(_lib.ptr(qp), _lib.ptr(db.blob), _lib.ptr(small.blob), _lib.ptr(qlp), 1, 3, 32769, 64,
                                       _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr())
    assert rcode == _lib.WV_ENOTSUP and b"outside the windowed kernel" in lib.wv_last_error()
    assert not bool(out.any())
    # three label words: None, like hamming_map_at_k
    wide = torch.zeros((100, 3), dtype=torch.int64, device="cuda")
    db100 = H.PreparedDB(rp[:100].contiguous(), 64)
    assert H.hamming_radius_hist(qp, db100, H.PreparedLabels(wide), torch.zeros((3, 3), dtype=torch.int64, device="cuda"), 64) is None


def test_cum_is_hamming_hist_bit_for_bit():
    q, r, ql, rl = rc.make_inputs(67, 5000, 64, 38, seed=3)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    db = H.PreparedDB(rp, 64)
    cum, _ = H.hamming_radius_hist(qp, db, H.PreparedLabels(H.pack_labels(rl.cuda())), H.pack_labels(ql.cuda()), 64)
    assert torch.equal(cum, H.hamming_hist(qp, db, 64))


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_golden_through_the_gpu_wrappers_and_the_calculator(golden_dir, name, tmp_path, monkeypatch):
    g = rc.load_golden(golden_dir, name)
    q, r, ql, rl = g["q"], g["r"], g["ql"], g["rl"]
    tol = rc.golden_tol(q.shape[0])
    ql_before = ql.clone()
    P, R = RM.pr_curve(q.cuda(), r.cuda(), ql.cuda(), rl.cuda())
    assert P.is_cuda and P.dtype == torch.float64
    errs = [np.abs(P.cpu().numpy() - g["ref_P"]).max(), np.abs(R.cpu().numpy() - g["ref_R"]).max()]
    for rad, want in zip(g["radii"], g["ref_prec"]):
        errs.append(abs(RM.get_precision_recall_by_Hamming_Radius(r, rl, q, ql, radius=rad) - float(want)))   # host tensors are moved
    # the calculator, alone and sharing a RankCache: the same numbers
    monkeypatch.chdir(tmp_path)
    qc, rcd, qlc, rlc = q.cuda(), r.cuda(), ql.cuda(), rl.cuda()
    outs = []
    for cache in (None, RankCache()):
        calc = CustomCalculator(include=("precision_hamming_radius", "pr_curve_hamming"), hamming_radius=g["radii"][1], rank_cache=cache)
        out = calc.get_accuracy(qc, qlc, rcd, rlc, False)
        assert set(out) == {"precision_hamming_radius", "pr_curve_hamming"} and out["pr_curve_hamming"] == 0
        outs.append((out["precision_hamming_radius"], calc.last_pr_curve_hamming))
        errs.append(abs(out["precision_hamming_radius"] - float(g["ref_prec"][1])))
        assert torch.equal(calc.last_pr_curve_hamming[0], P) and torch.equal(calc.last_pr_curve_hamming[1], R)
    assert outs[0][0] == outs[1][0]
    print(f"{name}: tol={tol:.3e} errors {[f'{e:.2e}' for e in errs]}")
    assert max(errs) <= tol, (errs, tol)
    assert os.listdir(tmp_path) == [] and torch.equal(ql, ql_before)
    plain = CustomCalculator(k=10, distance_metric="hamming", with_faiss=False)
    assert not {"precision_hamming_radius", "pr_curve_hamming"} & set(plain.get_curr_metrics())
