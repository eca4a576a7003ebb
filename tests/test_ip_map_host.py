"""wv_ip_map_at_k_cpu, the host twin of the batch mAP proxy (csrc/host_ip_map.cpp), and what is built on it without a GPU:
against the oracle on inputs whose fp32 arithmetic is exact, against the composition the contract is defined by
(wv_knn_float_cpu(IP, k) + wv_map_at_k_cpu), against the Hamming ranking on +-1 codes, the closed form when every score is
equal, every argument refusal, and CustomCalculator(device='cpu') with soft_codes."""
import ctypes
import os
import re

import pytest
import torch

import ip_map_cases as C
from oracle import ranking
from wvhash import _lib
from wvhash.engine import CustomCalculator, hamming as H, hamming_host as HH
from wvhash.engine.get_knn import knn_float_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin(case):
    x = C.inputs(case)
    got = HH.ip_map_at_k(x.q, x.db, x.qlp, x.rlp, x.k)
    assert got is not None
    ap, nrel = got
    assert ap.dtype == torch.float32 and nrel.dtype == torch.int32 and ap.shape == nrel.shape == (case.Q,)
    return ap, nrel


def assert_bits(a, b):
    assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), (a, b)


@pytest.mark.parametrize("case", C.EXACT_CASES + C.WORD2_CASES, ids=C.case_id)
def test_twin_matches_the_oracle_on_exact_inputs(case):
    ap, nrel = twin(case)
    ref_ap, ref_hits = C.oracle_ap(case)
    print(case, "max |ap - oracle| =", float((ap.double() - ref_ap).abs().max()))
    assert torch.equal(nrel, ref_hits)
    assert float((ap.double() - ref_ap).abs().max()) <= C.AP_TOL


def test_hits_in_the_second_label_word_are_seen():
    case = C.WORD2_CASES[0]
    x = C.inputs(case)
    assert int(x.qlp[:, 0].abs().sum()) == 0 and int(x.rlp[:, 0].abs().sum()) == 0 and int(x.rlp[:, 1].ne(0).sum()) > 0
    assert int(twin(case)[1][0]) == int(x.rl.sum(1).gt(0).sum())      # query 0 carries every used class


@pytest.mark.parametrize("case", C.COMPOSED_CASES, ids=C.case_id)
def test_twin_is_map_at_k_of_the_knn_list_bit_for_bit(case):
    x = C.inputs(case)
    ap, nrel = twin(case)
    _, idx = knn_float_host(x.db, x.q, x.k, _lib.WV_METRIC_IP)
    ap2, nrel2 = HH.map_at_k(idx, x.qlp, x.rlp, k=x.k)
    assert_bits(ap, ap2)
    assert torch.equal(nrel, nrel2)


@pytest.mark.parametrize("case", C.PM1_CASES, ids=C.case_id)
def test_on_pm1_codes_the_result_is_the_hamming_rankings(case):
    x = C.inputs(case)
    ap, nrel = twin(case)
    idx, _ = HH.hamming_topk(HH.pack_codes(x.q), HH.pack_codes(x.db), case.D, x.k)
    ap2, nrel2 = HH.map_at_k(idx, x.qlp, x.rlp, k=x.k)
    assert_bits(ap, ap2)
    assert torch.equal(nrel, nrel2)


@pytest.mark.parametrize("case", C.EQUAL_CASES, ids=C.case_id)
def test_equal_scores_rank_by_row(case):
    ap, nrel = twin(case)
    ref_ap, ref_hits = C.closed_form_equal(case)
    assert torch.equal(nrel, ref_hits) and int(nrel[-1]) == 0 and float(ap[-1]) == 0.0 and int(nrel[0]) > 0
    assert float((ap.double() - ref_ap).abs().max()) <= C.AP_TOL


def test_nrel_is_optional_and_no_query_is_no_work():
    lib = _lib.load()
    x = C.inputs(C.EXACT_CASES[4])
    ap = torch.full((x.q.shape[0],), -1.0)
    rc = lib.wv_ip_map_at_k_cpu(_lib.ptr(x.q), _lib.ptr(x.db), x.q.shape[0], x.db.shape[0], x.q.shape[1], _lib.ptr(x.qlp),
                                _lib.ptr(x.rlp), 1, x.k, _lib.ptr(ap), None)
    assert rc == 0
    assert_bits(ap, twin(C.EXACT_CASES[4])[0])
    one = ctypes.c_void_p(16)                          # never dereferenced: there is no query
    assert lib.wv_ip_map_at_k_cpu(one, one, 0, 10, 4, one, one, 1, 3, one, None) == 0
    assert lib.wv_ip_map_at_k(one, one, 0, 10, 4, one, one, 1, 3, one, None, None) == 0
    e = torch.empty((0, 16))
    ap0, nrel0 = HH.ip_map_at_k(e, torch.zeros(5, 16), torch.zeros((0, 1), dtype=torch.int64), torch.zeros((5, 1), dtype=torch.int64), 2)
    assert ap0.shape == nrel0.shape == (0,)


def _call(lib, gpu, q, db, Q, N, D, qlab, dblab, lwords, k, ap, nrel=None):
    if gpu:
        return lib.wv_ip_map_at_k(q, db, Q, N, D, qlab, dblab, lwords, k, ap, nrel, None)
    return lib.wv_ip_map_at_k_cpu(q, db, Q, N, D, qlab, dblab, lwords, k, ap, nrel)


@pytest.mark.parametrize("gpu", [False, True], ids=["twin", "kernel-entry"])
def test_arguments_are_refused_on_the_host(gpu):
    """Every refusal is answered before a pointer is read or anything is launched: the pointers here are never dereferenced,
    and the kernel's entry point answers on a machine without a GPU."""
    lib = _lib.load()
    one, null = ctypes.c_void_p(16), None
    name = b"ip_map_at_k:" if gpu else b"ip_map_at_k_cpu:"
    good = dict(q=one, db=one, Q=4, N=100, D=16, qlab=one, dblab=one, lwords=1, k=10, ap=one)
    refusals = [({"Q": -1}, b"Q=-1"), ({"N": 0}, b"N=0"), ({"N": -3}, b"N=-3"), ({"D": 0}, b"D=0"), ({"k": 0}, b"k=0"),
                ({"k": -2}, b"k=-2"), ({"k": 101}, b"k=101"), ({"lwords": 0}, b"lwords=0"), ({"lwords": 3}, b"lwords=3"),
                ({"q": null}, b"q is null"), ({"db": null}, b"db is null"), ({"qlab": null}, b"qlab is null"),
                ({"dblab": null}, b"dblab is null"), ({"ap": null}, b"ap is null")]
    for change, text in refusals:
        assert _call(lib, gpu, **{**good, **change}) == -22, change
        msg = lib.wv_last_error()
        assert text in msg and msg.startswith(name), (change, msg)
    rows = _lib.WV_IP_MAP_ROWS_MAX
    assert _call(lib, gpu, **{**good, "N": rows + 1}) == -95
    assert b"WV_IP_MAP_ROWS_MAX=%d" % rows in lib.wv_last_error() and b"N=%d" % (rows + 1) in lib.wv_last_error()
    assert _call(lib, gpu, **{**good, "D": 513}) == -95 and b"D=513" in lib.wv_last_error() and b"512" in lib.wv_last_error()
    assert _call(lib, gpu, **{**good, "N": rows + 1, "k": rows + 2}) == -22        # a bad argument before an unsupported shape


def test_the_row_limit_is_one_constant():
    txt = open(os.path.join(ROOT, "include", "wvhash.h")).read()
    (value,) = re.findall(r"#define WV_IP_MAP_ROWS_MAX (\d+)", txt)
    assert int(value) == _lib.WV_IP_MAP_ROWS_MAX == H.IP_MAP_ROWS_MAX == HH.IP_MAP_ROWS_MAX >= 2048


def test_wrapper_answers_none_outside_the_limits_and_widens_half_precision():
    q, ql = C.same_source(8, 16, 1)
    big = C.grid_embeddings(HH.IP_MAP_ROWS_MAX + 1, 16, 3)
    lab = torch.zeros((big.shape[0], 1), dtype=torch.int64)
    assert HH.ip_map_at_k(q, big, C.pack_bits(ql), lab, 5) is None
    wide = torch.zeros((8, 3), dtype=torch.int64)
    assert HH.ip_map_at_k(q, q, wide, wide, 5) is None                                  # labels of more than two words
    qlp = C.pack_bits(ql)
    for half in (torch.bfloat16, torch.float16):                                         # both hold the 2^-8 grid exactly
        assert_bits(HH.ip_map_at_k(q.to(half), q.to(half), qlp, qlp, 5)[0], HH.ip_map_at_k(q, q, qlp, qlp, 5)[0])
    with pytest.raises(ValueError, match="ip_map_at_k: q: expected dtype"):
        HH.ip_map_at_k(q.double(), q, qlp, qlp, 5)
    with pytest.raises(ValueError, match="ip_map_at_k: db: expected shape"):
        HH.ip_map_at_k(q, q[:, :8], qlp, qlp, 5)
    with pytest.raises(ValueError, match="k=9"):
        HH.ip_map_at_k(q, q, qlp, qlp, 9)


# ---------------------------------------------------------------------------------------------- CustomCalculator(device='cpu')
def _calc(soft):
    calc = CustomCalculator(exclude=["NMI", "AMI"], k="max_bin_count", with_faiss=False, distance_metric="hamming", device="cpu")
    calc.soft_codes = soft
    return calc


def test_soft_codes_defaults_to_false_and_real_values_still_raise():
    emb, lab = C.same_source(96, 64, 1)
    calc = CustomCalculator(k="max_bin_count", with_faiss=False, distance_metric="hamming", device="cpu")
    assert calc.soft_codes is False
    with pytest.raises(ValueError, match="exactly"):
        calc.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True)
    zero = C.pm1_codes(8, 16, 1)
    zero[0, 0] = 0.0                                                                     # sign(0)
    with pytest.raises(ValueError, match="exactly"):
        calc.calculate_maphashing(zero, lab[:8], zero, lab[:8], 4)


@pytest.mark.parametrize("lwords", [1, 2])
def test_soft_codes_same_source_batch_matches_the_oracle(lwords):
    emb, lab = C.same_source(96, 64, lwords)
    got, per_query = _calc(True).calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True,
                                                      return_per_query=True)
    ref, ref_pq = ranking.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True, stable=True,
                                               return_per_query=True)
    assert ref > 0.0
    assert abs(got - ref) <= C.AP_TOL
    assert float((per_query.double() - torch.tensor(ref_pq, dtype=torch.float64)).abs().max()) <= C.AP_TOL


def test_soft_codes_beyond_the_fused_limit_takes_the_composed_path(monkeypatch):
    q, ql = C.same_source(6, 64, 1, seed=21)
    db, rl = C.same_source(3000, 64, 1, seed=23)
    answers = []
    fused = HH.ip_map_at_k
    monkeypatch.setattr(HH, "ip_map_at_k", lambda *a: answers.append(fused(*a)) or answers[-1])
    got = _calc(True).calculate_maphashing(q, ql, db, rl, 500)
    assert answers == [None]                                                            # asked once, refused: 3000 > 2048 rows
    assert abs(got - ranking.calculate_maphashing(q, ql, db, rl, 500, stable=True)) <= C.AP_TOL


def test_soft_codes_leaves_pm1_codes_on_the_packed_path(monkeypatch):
    codes, lab = C.pm1_codes(96, 64, 31), C.multi_hot(96, 38, 0.10, 32)
    monkeypatch.setattr(HH, "ip_map_at_k", lambda *a: pytest.fail("+-1 codes must not take the inner-product path"))
    a = _calc(True).calculate_maphashing(codes, lab, codes, lab, "max_bin_count", ref_includes_query=True, return_per_query=True)
    b = _calc(False).calculate_maphashing(codes, lab, codes, lab, "max_bin_count", ref_includes_query=True, return_per_query=True)
    assert a[0] == b[0]
    assert_bits(a[1], b[1])


def test_soft_codes_several_cutoffs_make_one_call_each(monkeypatch):
    emb, lab = C.same_source(96, 64, 1)
    calls = []
    fused = HH.ip_map_at_k
    monkeypatch.setattr(HH, "ip_map_at_k", lambda *a: calls.append(a[-1]) or fused(*a))
    calc = _calc(True)
    got = calc.calculate_maphashing_at(emb, lab, emb, lab, [5, 50, 5])
    assert sorted(calls) == [5, 50]
    for k in (5, 50):
        assert abs(got[k] - ranking.calculate_maphashing(emb, lab, emb, lab, k, stable=True)) <= C.AP_TOL


def test_a_resolved_topk_of_zero_is_zero_without_a_call(monkeypatch):
    emb, _ = C.same_source(5, 16, 1)
    lab = torch.eye(5)                                                                  # no two rows share a tag
    monkeypatch.setattr(HH, "ip_map_at_k", lambda *a: pytest.fail("nothing to rank"))
    calc = _calc(True)
    assert calc.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True) == 0.0
    value, per_query = calc.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True, return_per_query=True)
    assert value == 0.0 and per_query.shape == (5,) and not per_query.any()
    assert ranking.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True, stable=True) == 0.0
