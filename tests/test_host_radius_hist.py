"""Precision / recall by Hamming radius on the CPU box: the host twin wv_hamming_radius_hist_cpu against a brute-force
expectation (exact), the metrics of wvhash/engine/radius_metrics.py and CustomCalculator(device='cpu') against values the
REFERENCE's own pr_curve / get_precision_recall_by_Hamming_Radius produced (main/engine/DSCH/_utils.py:469-493, 577-594;
tests/golden/radius_golden.npz), and the sharded form over real gloo ranks.  No GPU is touched."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import radius_cases as rc
from wvhash import _lib
from wvhash.engine import CustomCalculator, get_accuracy_calculator
from wvhash.engine import hamming_host as HH
from wvhash.engine import radius_metrics as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wv_hamming_radius_hist", "wv_hamming_radius_hist_cpu")


def _twin(q, r, ql, rl):
    return HH.hamming_radius_hist(HH.pack_codes(q), HH.pack_codes(r), HH.pack_labels(rl), HH.pack_labels(ql), q.shape[1])


def test_header_declares_and_both_libraries_export_the_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wvhash.h")).read(), flags=re.S)
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for s in NEW:
            assert re.search(rf"\bint {s}\s*\(", txt), f"{s} not declared"
            assert re.search(rf"\bT {s}$", exported, flags=re.M), f"{s} not exported by {path}"
    assert _lib.load().wv_abi_version() == 5


@pytest.mark.parametrize("Q,N,nbits,classes", [(1, 1, 16, 12), (5, 255, 48, 12), (9, 257, 64, 80), (7, 4097, 128, 80),
                                               (3, 40000, 64, 12), (4, 300, 1, 5), (6, 64, 100, 70)])
def test_twin_tables_equal_brute_force(Q, N, nbits, classes):
    q, r, ql, rl = rc.make_inputs(Q, N, nbits, classes, seed=N + nbits)
    cum, cumrel = _twin(q, r, ql, rl)
    want = rc.brute_tables(q, r, ql, rl)
    assert cum.dtype == torch.int32 and tuple(cum.shape) == tuple(cumrel.shape) == (Q, nbits + 2)
    assert torch.equal(cum, want[0]) and torch.equal(cumrel, want[1])
    assert bool((cum[:, -1] == N).all()) and bool((cumrel[0] == 0).all())            # query 0 has no class
    if N >= 8:
        assert bool((cum[:min(Q, 4), 1] >= 2).all())                                 # the duplicate rows at distance 0
    if classes > 64:
        assert int(cumrel[Q - 1, -1]) > 0                                            # classes of the second label word only
    # cum = what the distance twin gives, counted (wv_hamming_hist's numbers)
    d = HH.hamming_dist(HH.pack_codes(q), HH.pack_codes(r), nbits).long()
    hist = torch.zeros((Q, nbits + 2), dtype=torch.long).scatter_add_(1, d + 1, torch.ones_like(d))
    assert torch.equal(cum.long(), hist.cumsum(1))


def test_twin_refuses_what_it_does_not_cover():
    q, r, ql, rl = rc.make_inputs(3, 20, 64, 12, seed=1)
    lib = _lib.load()
    qp, rp, qlp, rlp = HH.pack_codes(q), HH.pack_codes(r), HH.pack_labels(ql), HH.pack_labels(rl)
    out = torch.zeros((3, 66), dtype=torch.int32)
    args = (_lib.ptr(qp), _lib.ptr(rp), _lib.ptr(qlp), _lib.ptr(rlp))
    assert lib.wv_hamming_radius_hist_cpu(*args, 3, 3, 20, 64, _lib.ptr(out), _lib.ptr(out)) == -22 and b"lwords" in lib.wv_last_error()
    assert lib.wv_hamming_radius_hist_cpu(*args, 1, 3, 20, 129, _lib.ptr(out), _lib.ptr(out)) == -22
    assert lib.wv_hamming_radius_hist_cpu(*args, 1, 3, 20, 64, None, _lib.ptr(out)) == -22
    one = __import__("ctypes").c_void_p(16)                # never dereferenced: the GPU entry point validates on the host
    assert lib.wv_hamming_radius_hist(one, one, one, one, 1, 4, 0, 64, one, one, None) == -22
    assert lib.wv_hamming_radius_hist(one, one, one, one, 1, 4, 100, 129, one, one, None) == -22
    assert lib.wv_hamming_radius_hist(one, one, one, one, 3, 4, 100, 64, one, one, None) == -95
    assert lib.wv_hamming_radius_hist(one, one, one, one, 1, 4, 32769, 64, one, one, None) == -95
    assert b"32769 rows" in lib.wv_last_error() and b"outside the windowed kernel" in lib.wv_last_error()
    wide = torch.zeros((20, 3), dtype=torch.int64)
    assert HH.hamming_radius_hist(qp, rp, wide, torch.zeros((3, 3), dtype=torch.int64), 64) is None


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_metrics_reproduce_the_reference_made_values(golden_dir, name):
    g = rc.load_golden(golden_dir, name)
    Q, tol = g["q"].shape[0], rc.golden_tol(g["q"].shape[0])
    tables = _twin(g["q"], g["r"], g["ql"], g["rl"])
    P, R = RM.radius_curves(*tables)
    assert P.dtype == torch.float64 and tuple(P.shape) == tuple(R.shape) == (g["nbits"] + 1,)
    errs = [np.abs(P.numpy() - g["ref_P"]).max(), np.abs(R.numpy() - g["ref_R"]).max()]
    ql_before = g["ql"].clone()
    P2, R2 = RM.pr_curve(g["q"], g["r"], g["ql"], g["rl"], device="cpu")
    assert torch.equal(P2, P) and torch.equal(R2, R)
    for rad, want in zip(g["radii"], g["ref_prec"]):
        got = RM.precision_within_radius(*tables, radius=rad)
        via = RM.get_precision_recall_by_Hamming_Radius(g["r"].numpy(), g["rl"].numpy(), g["q"].numpy(), g["ql"].numpy(), radius=rad,
                                                        device="cpu")
        assert via == got
        errs.append(abs(got - float(want)))
    print(f"{name}: Q={Q} tol={tol:.3e} |P|,|R|,|prec| errors {[f'{e:.2e}' for e in errs]}")
    assert max(errs) <= tol, (errs, tol)
    assert torch.equal(g["ql"], ql_before)                 # the reference overwrites the zeros of query_labels with -1; we do not


def test_wrappers_need_a_gpu_or_an_explicit_cpu():
    g = rc.make_inputs(3, 20, 32, 5, seed=2)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.WvhashUnavailable):
            RM.pr_curve(g[0], g[1], g[2], g[3])
        with pytest.raises(_lib.WvhashUnavailable):
            RM.get_precision_recall_by_Hamming_Radius(g[1], g[3], g[0], g[2])
    with pytest.raises(ValueError, match="exactly"):
        RM.pr_curve(torch.zeros(3, 32), g[1], g[2], g[3], device="cpu")
    with pytest.raises(ValueError, match="128"):
        RM.pr_curve(torch.ones(3, 192), torch.ones(20, 192), g[2], g[3], device="cpu")


def test_calculator_metrics_are_opt_in(golden_dir, tmp_path, monkeypatch):
    name = "c64_q32_n1000_k38"
    g = rc.load_golden(golden_dir, name)
    q, r, ql, rl = g["q"], g["r"], g["ql"], g["rl"]
    tol = rc.golden_tol(q.shape[0])
    # absent unless named: the key set of tests/test_host_rank.py's c0 run
    exclude = ["mean_reciprocal_rank", "mean_average_precision", "mean_average_precision_at_r", "precision_at_1", "recall_at_1",
               "r_precision", "rpr", "pr", "pr_rc", "recall_at_1000", "recall_at_100", "recall_at_10", "recall_at_16", "recall_at_20",
               "recall_at_30", "recall_at_32", "recall_at_4", "recall_at_8", "recall_at_2"]
    calc = get_accuracy_calculator(k=50, device=torch.device("cpu"), distance_metric="hamming", with_faiss=False, exclude=exclude)
    assert set(calc.get_accuracy(q, ql, r, rl, False)) == {"maphashing", "map", "bit_balance", "worst_bit_balance"}
    plain = CustomCalculator(k=50, device="cpu", distance_metric="hamming", with_faiss=False)
    assert not {"precision_hamming_radius", "pr_curve_hamming"} & set(plain.get_curr_metrics())
    assert not {"precision_hamming_radius", "pr_curve_hamming"} & set(plain.get_accuracy(q, ql, r, rl, False, include=("maphashing", "bit_balance")))
    # named in get_accuracy
    ql_before = ql.clone()
    monkeypatch.chdir(tmp_path)                            # a stray default-path file would land here
    out = plain.get_accuracy(q, ql, r, rl, False, include=("precision_hamming_radius", "pr_curve_hamming"))
    assert set(out) == {"precision_hamming_radius", "pr_curve_hamming"} and out["pr_curve_hamming"] == 0
    assert abs(out["precision_hamming_radius"] - float(g["ref_prec"][1])) <= tol
    P, R = plain.last_pr_curve_hamming
    assert np.abs(P.numpy() - g["ref_P"]).max() <= tol and np.abs(R.numpy() - g["ref_R"]).max() <= tol
    assert os.listdir(tmp_path) == [] and torch.equal(ql, ql_before)          # no path, no file; labels untouched
    # named at construction, with a radius and a path of their own
    path = os.path.join(tmp_path, "curve.csv")
    calc2 = CustomCalculator(include=("pr_curve_hamming", "precision_hamming_radius"), device="cpu", hamming_radius=g["radii"][2],
                             pr_curve_hamming_path=path)
    out2 = calc2.get_accuracy(q, ql, r, rl, False)
    assert set(out2) == {"precision_hamming_radius", "pr_curve_hamming"}
    assert abs(out2["precision_hamming_radius"] - float(g["ref_prec"][2])) <= tol
    import pandas as pd
    csv = pd.read_csv(path)
    assert list(csv.columns) == ["radius", "pr", "rc"] and list(csv["radius"]) == list(range(g["nbits"] + 1))
    np.testing.assert_allclose(csv["pr"].to_numpy(), P.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(csv["rc"].to_numpy(), R.numpy(), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="at most 128 bits"):
        calc2.calculate_precision_hamming_radius(torch.ones(2, 192), ql[:2], torch.ones(5, 192), rl[:5])
    with pytest.raises(ValueError, match="at most 128 bits"):
        calc2.calculate_pr_curve_hamming(torch.zeros(2, 64), ql[:2], r[:5], rl[:5])


# ----------------------------------------------------------------------------------------- sharded, gloo
GLOO_CASES = [(1001, 64, 12), (700, 128, 80)]              # N not divisible by 2 or 3; 128-bit codes with two label words


def _gloo_inputs(world, ql, n_db, nbits, classes):
    return rc.make_inputs(world * ql, n_db, nbits, classes, seed=n_db + nbits)


def _radius_worker(rank, world, port, cases, ql, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "image-retrieval-wavelet_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from wvhash import parallel
    out = {}
    for n_db, nbits, classes in cases:
        q, r, qlab, rlab = _gloo_inputs(world, ql, n_db, nbits, classes)
        lo, hi, _ = parallel.shard_bounds(n_db, world, rank)
        sl = slice(rank * ql, (rank + 1) * ql)
        parallel.TRACE = parallel.ExchangeTrace()
        out[(n_db, nbits)] = parallel.sharded_hamming_radius_hist(HH.pack_codes(q[sl]), HH.pack_labels(qlab[sl]), HH.pack_codes(r[lo:hi]),
                                                                  HH.pack_labels(rlab[lo:hi]), nbits)
        calls, parallel.TRACE = parallel.TRACE.calls, None
        assert calls == {"all_gather": 1, "all_reduce": 1, "all_to_all": 0}, calls
    torch.save(out, os.path.join(out_dir, f"rad{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,cases", [(2, GLOO_CASES), (3, GLOO_CASES + [(4, 64, 12)])])   # 4 rows on 3 ranks: an empty last shard
def test_sharded_tables_equal_the_unsharded_twin(tmp_path, world, cases):
    ql = 4
    port = 35700 + (os.getpid() + world * 17) % 2000
    mp.spawn(_radius_worker, args=(world, port, cases, ql, str(tmp_path)), nprocs=world, join=True)
    for n_db, nbits, classes in cases:
        q, r, qlab, rlab = _gloo_inputs(world, ql, n_db, nbits, classes)
        want = _twin(q, r, qlab, rlab)
        for rank in range(world):
            got = torch.load(os.path.join(tmp_path, f"rad{rank}.pt"))[(n_db, nbits)]
            assert got[0].dtype == torch.int32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (world, rank, n_db)
