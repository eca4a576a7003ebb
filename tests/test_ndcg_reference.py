"""NDCG and precision at top-K against values the REFERENCE's own code produced (tests/golden/ndcg_golden.npz, made by
tests/golden/make_golden_ndcg.py from main/engine/DSCH/_utils.py:496-574).  CPU only: the definitions restated in numpy, the
interval tie-breaking can produce, and the host twins behind device='cpu'.

The reference ranks with an unstable sort, wvhash by (distance, row): on tied distances the two legitimately differ, by
exactly the orderings ndcg_tie_bounds / ptopk_tie_bounds enumerate.  Where the order is pinned (the recorded order, or a
tie-free case) the values agree to the derived ndcg_tol."""
import functools

import numpy as np
import pytest
import torch

import ndcg_cases as C
from conftest import GOLDEN
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming_host as HH
from wvhash.engine import ndcg as ND


@functools.lru_cache(maxsize=None)
def case(name):
    c = C.load_golden(GOLDEN, name)
    c["Rel"] = C.overlaps(c["ql"].numpy(), c["rl"].numpy())
    c["d"] = C.scores_np(c)
    c["N"] = c["r"].shape[0]
    c["canon"] = C.canonical_order(c["d"])
    return c


def cut(c, k):
    return c["N"] if k < 0 else k


@pytest.mark.parametrize("name", C.HAMMING_CASES + C.REAL_CASES)
def test_restatement_on_the_recorded_order_is_the_reference_value(name):
    c, checked = case(name), 0
    for k, ref in zip(c["ks"], c["ref_ndcg"]):
        kk = cut(c, k)
        if kk <= c["order"].shape[1]:                         # the stored columns of the recorded order reach this cut-off
            assert abs(C.ndcg_restated(c["order"], c["Rel"], kk) - ref) <= C.ndcg_tol(kk), (name, k)
            checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", C.HAMMING_CASES + C.REAL_CASES)
def test_reference_values_lie_inside_the_tie_bounds(name):
    c = case(name)
    for k, ref in zip(c["ks"], c["ref_ndcg"]):
        kk = cut(c, k)
        lo, hi = C.ndcg_tie_bounds(c["d"], c["Rel"], kk)
        assert lo - C.ndcg_tol(kk) <= ref <= hi + C.ndcg_tol(kk), (name, k, lo, ref, hi)
        canon = C.ndcg_restated(c["canon"], c["Rel"], kk)
        assert lo - C.ndcg_tol(kk) <= canon <= hi + C.ndcg_tol(kk), (name, k, lo, canon, hi)
    if c["what"] == 1:
        Q = c["q"].shape[0]
        lo, hi = C.ptopk_tie_bounds(c["d"], c["Rel"] > 0, c["K"])
        assert np.all(lo - C.ptopk_tol(Q) <= c["ref_ptopk"]) and np.all(c["ref_ptopk"] <= hi + C.ptopk_tol(Q)), (name, lo, hi)


@pytest.mark.parametrize("name", C.HAMMING_CASES)
def test_host_ndcg_hamming_inside_bounds_and_equal_to_the_canonical_restatement(name):
    c = case(name)
    for k in c["ks"]:
        kk = cut(c, k)
        got = ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=1, k=k, device="cpu")
        lo, hi = C.ndcg_tie_bounds(c["d"], c["Rel"], kk)
        assert lo - C.ndcg_tol(kk) <= got <= hi + C.ndcg_tol(kk), (name, k, lo, got, hi)
        assert abs(got - C.ndcg_restated(c["canon"], c["Rel"], kk)) <= C.ndcg_tol(kk), (name, k)
    many = ND.ndcg_at(c["q"], c["r"], c["ql"], c["rl"], [cut(c, k) for k in c["ks"]] + [10 ** 6], what=1, device="cpu")
    assert many.dtype == torch.float64 and many.shape == (len(c["ks"]) + 1,)
    for k, v in zip(c["ks"], many):
        assert abs(float(v) - ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=1, k=k, device="cpu")) <= 2.0 ** -52
    assert float(many[-1]) == float(many[-2])                  # a cut-off beyond the database clips at N (= k -1)


@pytest.mark.parametrize("name", C.REAL_CASES)
def test_host_tie_free_cases_equal_the_reference(name):
    c = case(name)
    qlp, rlp = HH.pack_labels(c["ql"]), HH.pack_labels(c["rl"])
    order = torch.from_numpy(c["order"].astype(np.int32))
    assert order.shape[1] == c["N"]
    for k, ref in zip(c["ks"], c["ref_ndcg"]):
        kk = cut(c, k)
        fed = float(ND.ndcg_from_sums(*HH.ndcg_at_ks(order, qlp, rlp, [kk]))[0])       # the twin fed the stored order
        assert abs(fed - ref) <= C.ndcg_tol(kk), (name, k, fed, ref)
        own = ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=c["what"], k=k, device="cpu")   # ... and its own fp32 ranking
        assert abs(own - ref) <= C.ndcg_tol(kk), (name, k, own, ref)


@pytest.mark.parametrize("name", C.HAMMING_CASES)
def test_host_p_topk_inside_bounds(name):
    c = case(name)
    Q = c["q"].shape[0]
    K = c["K"] + [c["N"] + 5, c["K"][0]]                       # a cut-off beyond N and a repeat: clamped, mapped back
    got = ND.p_topK(c["q"], c["r"], c["ql"], c["rl"], K=K, device="cpu")
    assert got.dtype == torch.float64 and got.shape == (len(K),)
    lo, hi = C.ptopk_tie_bounds(c["d"], c["Rel"] > 0, c["K"])
    g = got.numpy()
    assert np.all(lo - 2.0 ** -50 <= g[:4]) and np.all(g[:4] <= hi + 2.0 ** -50), (name, lo, g, hi)
    assert g[4] == g[3] and g[5] == g[0]
    # K = N: every ordering keeps the same rows -- the reference's value itself, to its fp32 rounding
    assert abs(g[3] - c["ref_ptopk"][3]) <= C.ptopk_tol(Q)
    assert ND.p_topK(c["q"], c["r"], c["ql"], c["rl"], device="cpu").shape == (11,)        # the reference's default K list


def test_calculator_metric_is_opt_in_and_equals_the_function():
    c = case("c32_q16_n300_k12")
    args = (c["q"], c["ql"], c["r"], c["rl"])
    plain = CustomCalculator(k=50, distance_metric="hamming", with_faiss=False, device="cpu", include=("maphashing",))
    assert "ndcg_hamming" not in plain.get_accuracy(*args, False)
    assert "ndcg_hamming" not in CustomCalculator(k=50, distance_metric="hamming", with_faiss=False, device="cpu",
                                                  exclude=("pr_rc", "pr_rc_hashing")).get_curr_metrics()
    for ndcg_k, k in ((None, 300), (50, 50), (-1, 300), (1000, 300)):
        kw = {} if ndcg_k is None else {"ndcg_k": ndcg_k}
        calc = CustomCalculator(k=50, distance_metric="hamming", with_faiss=False, device="cpu",
                                include=("maphashing", "ndcg_hamming"), **kw)
        assert calc.ndcg_k == (1000 if ndcg_k is None else ndcg_k)
        got = calc.get_accuracy(*args, False)
        assert set(got) == {"maphashing", "ndcg_hamming"}
        assert got["ndcg_hamming"] == ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=1, k=k, device="cpu")
    named = plain.get_accuracy(*args, False, include=("ndcg_hamming",))                   # nameable per call as well
    assert named == {"ndcg_hamming": ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=1, k=1000, device="cpu")}


def test_ndcg_from_sums_divides_by_all_queries_and_skips_lone_ones():
    dcg = torch.tensor([[1.0, 2.0], [0.0, 0.0], [3.0, 3.0]], dtype=torch.float64)
    idcg = torch.tensor([[2.0, 4.0], [0.0, 0.0], [3.0, 6.0]], dtype=torch.float64)
    out = ND.ndcg_from_sums(dcg, idcg)
    assert out.dtype == torch.float64 and torch.equal(out, torch.tensor([1.5 / 3, 1.0 / 3], dtype=torch.float64))
    with pytest.raises(ValueError):
        ND.ndcg_from_sums(dcg, idcg[:, :1])
    with pytest.raises(ValueError):
        ND.NDCG(torch.ones(2, 8), torch.ones(3, 8), torch.ones(2, 3), torch.ones(3, 3), what=5, device="cpu")
    with pytest.raises(ValueError):                            # codes must be exactly +-1
        ND.NDCG(torch.zeros(2, 8), torch.ones(3, 8), torch.ones(2, 3), torch.ones(3, 3), what=1, device="cpu")
