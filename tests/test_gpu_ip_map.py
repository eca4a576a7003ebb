"""wv_ip_map_at_k on the GPU: the kernel's ap / nrel against the host twin's BIT FOR BIT on every case of
tests/ip_map_cases.py (tile edges of the 256-row staging, the sort's power-of-two padding, one and two label words, raw and
exact inputs, +-1 codes, all-equal scores), one batch against the oracle directly, the wrapper's argument gate, and
compute_batch_map on GPU batches."""
import pytest
import torch

import ip_map_cases as C
from oracle import ranking
from wvhash.engine import batch_map, hamming as H, hamming_host as HH

pytestmark = pytest.mark.gpu


def _dev(x):
    return [t.cuda() for t in (x.q, x.db, x.qlp, x.rlp)]


def _assert_same_bits(got, want):
    (ap, nrel), (ap_h, nrel_h) = got, want
    assert ap.dtype == torch.float32 and nrel.dtype == torch.int32
    assert torch.equal(nrel.cpu(), nrel_h)
    assert torch.equal(ap.cpu().view(torch.int32), ap_h.view(torch.int32)), (ap.cpu() - ap_h).abs().max()


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_kernel_equals_the_twin_bit_for_bit(case):
    x = C.inputs(case)
    got = H.ip_map_at_k(*_dev(x), x.k)
    assert got is not None
    _assert_same_bits(got, HH.ip_map_at_k(x.q, x.db, x.qlp, x.rlp, x.k))


def test_call_on_a_side_stream():
    case = C.COMPOSED_CASES[6]                                  # raw inputs, D = 64
    x = C.inputs(case)
    args = _dev(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = H.ip_map_at_k(*args, x.k)
    side.synchronize()
    _assert_same_bits(got, HH.ip_map_at_k(x.q, x.db, x.qlp, x.rlp, x.k))


def test_same_source_batch_against_the_oracle():
    emb, lab = C.same_source(256, 64, 1)
    lp = C.pack_bits(lab)
    k = 100
    ap, nrel = H.ip_map_at_k(emb.cuda(), emb.cuda(), lp.cuda(), lp.cuda(), k)
    _, per_query = ranking.calculate_maphashing(emb, lab, emb, lab, k, stable=True, return_per_query=True)
    order = torch.argsort(-(emb @ emb.t()), dim=1, stable=True)[:, :k]
    hits = torch.gather(ranking.label_comparison_fn(lab, lab), 1, order).sum(1).int()
    err = float((ap.cpu().double() - torch.tensor(per_query, dtype=torch.float64)).abs().max())
    print("B = 256, D = 64: max |ap - oracle| =", err)
    assert torch.equal(nrel.cpu(), hits) and int(hits.max()) > 1
    assert err <= C.AP_TOL


def test_wrapper_gate():
    """Every tensor passes engine/_args.gate: another device or dtype is refused with the wrapper's and the argument's name;
    a strided view is what the gate makes of it everywhere -- read as the contiguous tensor it denotes, never as raw memory;
    half-precision embeddings are widened (exact)."""
    emb, lab = C.same_source(96, 64, 1)
    lp = C.pack_bits(lab)
    q, l = emb.cuda(), lp.cuda()
    want = H.ip_map_at_k(q, q, l, l, 20)
    with pytest.raises(ValueError, match="ip_map_at_k: q: expected a tensor on a cuda device"):
        H.ip_map_at_k(emb, q, l, l, 20)
    for bad in ((q, emb, l, l), (q, q, lp, l), (q, q, l, lp)):
        with pytest.raises(ValueError, match="ip_map_at_k: .*lives on cpu"):
            H.ip_map_at_k(*bad, 20)
    with pytest.raises(ValueError, match="ip_map_at_k: q: expected dtype torch.float32"):
        H.ip_map_at_k(q.double(), q, l, l, 20)
    with pytest.raises(ValueError, match="ip_map_at_k: db: expected dtype torch.float32"):
        H.ip_map_at_k(q, q.long(), l, l, 20)
    with pytest.raises(ValueError, match="ip_map_at_k: qlab_packed: expected dtype torch.int64"):
        H.ip_map_at_k(q, q, l.int(), l, 20)
    with pytest.raises(ValueError, match="ip_map_at_k: dblab_packed: expected shape"):
        H.ip_map_at_k(q, q, l, l[:50], 20)
    wide = torch.zeros((96, 128), device="cuda")
    wide[:, ::2] = q
    strided_lab = torch.zeros((96, 2), dtype=torch.int64, device="cuda")
    strided_lab[:, :1] = l
    for form in ((wide[:, ::2], q, l, l), (q, q.t().contiguous().t(), l, l), (q, q, strided_lab[:, :1], l)):
        assert not all(t.is_contiguous() for t in form)
        _assert_same_bits(H.ip_map_at_k(*form, 20), tuple(t.cpu() for t in want))
    _assert_same_bits(H.ip_map_at_k(q.bfloat16(), q.half(), l, l, 20), tuple(t.cpu() for t in want))   # the 2^-8 grid fits both
    assert H.ip_map_at_k(q, torch.zeros((H.IP_MAP_ROWS_MAX + 1, 64), device="cuda"), l,
                         torch.zeros((H.IP_MAP_ROWS_MAX + 1, 1), dtype=torch.int64, device="cuda"), 20) is None


@pytest.mark.parametrize("B,lwords", [(96, 1), (1024, 2)])
def test_compute_batch_map_hamming_matches_the_oracle(B, lwords):
    calc, name = batch_map.build_batch_map_calculator("hamming", None)
    emb, lab = C.same_source(B, 64, lwords)
    got = batch_map.compute_batch_map(calc, name, emb.cuda(), lab.cuda())
    ref = ranking.calculate_maphashing(emb, lab, emb, lab, "max_bin_count", ref_includes_query=True, stable=True)
    print(f"B = {B}: proxy {got:.9f}, oracle {ref:.9f}")
    assert type(got) is float and ref > 0 and abs(got - ref) <= C.AP_TOL
    host = batch_map.compute_batch_map(batch_map.build_batch_map_calculator("hamming", "cpu")[0], name, emb, lab)
    assert abs(got - host) <= 1e-12                             # kernel and twin: the same APs; the fp64 means may round apart


def test_compute_batch_map_cosine_is_the_existing_knn_path():
    calc, name = batch_map.build_batch_map_calculator("cosine", None)
    emb, lab = C.same_source(96, 32, 1, kind="raw")
    emb = torch.nn.functional.normalize(emb, dim=1)
    got = batch_map.compute_batch_map(calc, name, emb.cuda(), lab.cuda())
    rel_all = ranking.label_comparison_fn(lab, lab)
    counts = rel_all.sum(1)
    num_k = int(counts.max()) - 1
    scores, idx = ranking.knn_stable(emb, emb, num_k + 1, "cosine")
    scores, idx = scores[:, 1:], idx[:, 1:]                     # the row itself leads its own list
    rel = torch.gather(rel_all, 1, idx)
    ref = ranking.retrieval_map(scores, rel, (counts - 1) > 0)
    assert name == "map" and ref > 0 and abs(got - ref) <= C.AP_TOL
