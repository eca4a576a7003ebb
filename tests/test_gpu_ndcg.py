"""The NDCG kernels (csrc/ndcg.hip) on the GPU: the overlap histogram equals the host twin exactly, DCG and ideal DCG equal the
twin's BIT FOR BIT (same table w, same summation order), a multi-cut column has the bits of the single-cut call, the
reference-made cases hold through NDCG / ndcg_at / p_topK, and one run at the c1 shape."""
import functools

import numpy as np
import pytest
import torch

import ndcg_cases as C
from conftest import GOLDEN
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming as H
from wvhash.engine import hamming_host as HH
from wvhash.engine import ndcg as ND

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("classes", C.HIST_CLASSES)
def test_overlap_hist_equals_the_twin(classes):
    for N in C.HIST_N:
        for Q in C.HIST_Q:
            ql, rl = C.make_labels(Q, N, classes, min(0.5, 3.0 / classes), 7 * N + Q)
            qlp, rlp = HH.pack_labels(ql), HH.pack_labels(rl)
            got = H.label_overlap_hist(qlp.cuda(), rlp.cuda())
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), HH.label_overlap_hist(qlp, rlp)), (classes, N, Q)


@pytest.mark.parametrize("classes", [38, 128])
def test_overlap_hist_edges_and_shards(classes):
    N, Q = 9000, 33                                            # three row slices, three query tiles, tails in both
    ql, rl = C.make_labels(Q, N, classes, 0.1, 3)
    rl[N - 1] = ql[1]                                          # the last row of the tail slice shares every class with query 1
    qlp, rlp = HH.pack_labels(ql).cuda(), HH.pack_labels(rl).cuda()
    whole = H.label_overlap_hist(qlp, rlp)
    assert torch.equal(whole.cpu(), HH.label_overlap_hist(qlp.cpu(), rlp.cpu()))        # the host twin takes host tensors
    assert int(whole[0, 0]) == N and int(whole[1, classes]) == 2 and bool((whole.sum(1) == N).all())
    assert torch.equal(H.label_overlap_hist(qlp, rlp[:4097]) + H.label_overlap_hist(qlp, rlp[4097:]), whole)
    same = HH.pack_labels(ql[2:3].repeat(N, 1)).cuda()         # one bin holds all N rows
    assert int(H.label_overlap_hist(qlp, same)[2, int(ql[2].sum())]) == N


@functools.lru_cache(maxsize=None)
def walk_inputs(classes, N=1200, Q=5):
    ql, rl = C.make_labels(Q, N, classes, min(0.5, 4.0 / classes), 11 + classes)
    ql[2] = 0                                                  # lone, like query 0
    if classes in (60, 128):                                   # query 1 and row 0 share every class; row 3 shares 60
        rl[3] = 0
        rl[3, :60] = 1
    idx = C.random_lists(Q, N, N, 5, absent=9)
    idx[:, 0] = torch.tensor([0, 0, 0, 3, 3])[:Q].int()
    qlp, rlp = HH.pack_labels(ql), HH.pack_labels(rl)
    return qlp, rlp, idx, qlp.cuda(), rlp.cuda(), idx.cuda()


@pytest.mark.parametrize("classes", [38, 60, 80, 128])
def test_walk_equals_the_twin_bit_for_bit(classes):
    qlp, rlp, idx, gq, gr, gi = walk_inputs(classes)
    N = rlp.shape[0]
    ghist = H.label_overlap_hist(gq, gr)
    hist = HH.label_overlap_hist(qlp, rlp)
    for ks in [[k] for k in C.WALK_KS + [N]] + [[255, 256, 257],
                                                 [1, 2, 63, 64, 65, 128, 255, 256, 257, 300, 511, 512, 513, 800, 1000, 1200]]:
        dcg, idcg = H.ndcg_at_ks(gi, gq, gr, ks, hist=ghist)
        want_d, want_i = HH.ndcg_at_ks(idx, qlp, rlp, ks, hist=hist)
        assert dcg.dtype == torch.float64 and torch.equal(bits(dcg), bits(want_d)), (classes, ks)
        assert torch.equal(bits(idcg), bits(want_i)), (classes, ks)
        assert float(dcg[2].abs().max()) == 0.0 and float(idcg[2].abs().max()) == 0.0     # the lone query
    made = H.ndcg_at_ks(gi, gq, gr, [1000])                    # the histogram made by the call itself
    assert torch.equal(bits(made[1]), bits(HH.ndcg_at_ks(idx, qlp, rlp, [1000])[1]))


def test_multi_cut_columns_have_the_bits_of_single_cut_calls():
    qlp, rlp, idx, gq, gr, gi = walk_inputs(80)
    ks = (100, 255, 256, 257, 1000)
    wide = torch.full((gi.shape[0], gi.shape[1] + 37), -7, dtype=torch.int32, device="cuda")   # ld > k_max
    wide[:, :gi.shape[1]] = gi
    dcg, idcg = H.ndcg_at_ks(wide[:, :max(ks) + 5], gq, gr, list(ks))
    for i, k in enumerate(ks):
        d1, i1 = H.ndcg_at_ks(gi, gq, gr, [k])
        assert torch.equal(bits(dcg[:, i]), bits(d1[:, 0])) and torch.equal(bits(idcg[:, i]), bits(i1[:, 0])), k


@functools.lru_cache(maxsize=None)
def case(name):
    c = C.load_golden(GOLDEN, name)
    c["Rel"] = C.overlaps(c["ql"].numpy(), c["rl"].numpy())
    c["d"] = C.scores_np(c)
    c["N"] = c["r"].shape[0]
    return c


@pytest.mark.parametrize("name", C.HAMMING_CASES + C.REAL_CASES)
def test_golden_cases(name):
    c = case(name)
    N, Q = c["N"], c["q"].shape[0]
    cuts = [N if k < 0 else k for k in c["ks"]]
    many = ND.ndcg_at(c["q"], c["r"], c["ql"], c["rl"], cuts, what=c["what"])
    assert many.is_cuda and many.dtype == torch.float64
    canon = C.canonical_order(c["d"])
    for k, kk, ref, got in zip(c["ks"], cuts, c["ref_ndcg"], many.cpu().tolist()):
        lo, hi = C.ndcg_tie_bounds(c["d"], c["Rel"], kk)
        assert lo - C.ndcg_tol(kk) <= got <= hi + C.ndcg_tol(kk), (name, k, lo, got, hi)
        assert abs(got - C.ndcg_restated(canon, c["Rel"], kk)) <= C.ndcg_tol(kk), (name, k)
        if c["what"] != 1:                                     # tie-free: the reference's value itself
            assert abs(got - ref) <= C.ndcg_tol(kk), (name, k, got, ref)
        # the twins sum the same bits (tested above); torch takes the mean over the queries in its own order per device
        assert abs(got - ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=c["what"], k=k, device="cpu")) <= C.mean_tol(Q)
    assert abs(ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=c["what"], k=-1) - many[-1].item()) <= C.mean_tol(Q)
    if c["what"] == 1:
        got = ND.p_topK(c["q"], c["r"], c["ql"], c["rl"], K=c["K"])
        assert got.is_cuda and got.dtype == torch.float64
        lo, hi = C.ptopk_tie_bounds(c["d"], c["Rel"] > 0, c["K"])
        g = got.cpu().numpy()
        assert np.all(lo - 2.0 ** -50 <= g) and np.all(g <= hi + 2.0 ** -50), (name, lo, g, hi)
        assert abs(g[3] - c["ref_ptopk"][3]) <= C.ptopk_tol(Q)
        assert torch.equal(got.cpu(), ND.p_topK(c["q"], c["r"], c["ql"], c["rl"], K=c["K"], device="cpu"))


def test_calculator_metric_on_the_gpu():
    from wvhash.engine.accuracy_calculator import RankCache
    c = case("c64_q32_n1000_k38")
    want = ND.NDCG(c["q"], c["r"], c["ql"], c["rl"], what=1, k=1000)
    args = tuple(t.cuda() for t in (c["q"], c["ql"], c["r"], c["rl"]))
    for cache in (None, RankCache()):
        calc = CustomCalculator(k=50, distance_metric="hamming", with_faiss=False, include=("maphashing", "ndcg_hamming"),
                                rank_cache=cache)
        got = calc.get_accuracy(*args, False)
        assert set(got) == {"maphashing", "ndcg_hamming"} and abs(got["ndcg_hamming"] - want) <= C.mean_tol(32)
    assert "ndcg_hamming" not in CustomCalculator(k=50, distance_metric="hamming", with_faiss=False,
                                                  include=("maphashing",)).get_accuracy(*args, False)


def test_c1_sized_run():
    from wvhash import synth
    Q, N, nbits, classes, k = 256, 25000, 64, 38, 1000
    ql, rl = synth.multi_hot_labels(Q, classes, 0.10, 1), synth.multi_hot_labels(N, classes, 0.10, 2)
    q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
    got = ND.ndcg_at(q, r, ql, rl, [100, k], what=1)
    assert bool(((got >= 0) & (got <= 1)).all()) and float(got[1]) > 0
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    idx = H.hamming_topk(qp, rp, nbits, k, want_dist=False)[0]
    hist = H.label_overlap_hist(qlp, rlp)
    assert bool((hist.sum(1) == N).all())
    dcg, idcg = H.ndcg_at_ks(idx, qlp, rlp, [100, k], hist=hist)
    assert float((ND.ndcg_from_sums(dcg, idcg) - got).abs().max()) <= C.mean_tol(Q)
    s = slice(100, 116)                                        # the twin on a 16-query slice
    assert torch.equal(hist[s].cpu(), HH.label_overlap_hist(qlp[s].cpu(), rlp.cpu()))
    want_d, want_i = HH.ndcg_at_ks(idx[s].cpu(), qlp[s].cpu(), rlp.cpu(), [100, k])
    assert torch.equal(bits(dcg[s]), bits(want_d)) and torch.equal(bits(idcg[s]), bits(want_i))
