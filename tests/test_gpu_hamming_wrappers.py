"""The Python wrappers of the Hamming ranking kernels (wvhash/engine/hamming.py) where they choose: hamming_topk's call forms
(one C entry point behind all of them) and the virtual-shard routes at their edges -- 32,769 rows, the first database that
is ranked as two parts, and a prefix longer than the windowed kernel's lists, which the fused mAP functions refuse while
hamming_topk still answers."""
import pytest
import torch

from oracle import ranking
from wvhash import synth
from wvhash.engine import hamming as H

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ hamming_topk's call forms
@pytest.fixture(scope="module", params=[64, 128])
def small(request):
    nbits = request.param
    q, r = synth.random_codes(5, 700, nbits, seed=nbits)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    prep = H.PreparedDB(rp, nbits)
    assert prep.parts is None
    return dict(nbits=nbits, q=q, r=r, qp=qp, rp=rp, prep=prep, cum=H.hamming_hist(qp, prep, nbits))


@pytest.mark.parametrize("k", [1, 37, 700])
def test_hamming_topk_call_forms_return_the_same_lists(small, k):
    """Packed tensor with and without a TopkWorkspace, PreparedDB, PreparedDB with want_cum: the same idx and dist, the
    oracle's; cum is hamming_hist's."""
    c = small
    ws = H.TopkWorkspace()
    forms = [H.hamming_topk(c["qp"], c["rp"], c["nbits"], k, workspace=ws), H.hamming_topk(c["qp"], c["rp"], c["nbits"], k),
             H.hamming_topk(c["qp"], c["prep"], c["nbits"], k), H.hamming_topk(c["qp"], c["prep"], c["nbits"], k, want_cum=True)]
    assert ws.buf is not None and [len(f) for f in forms] == [2, 2, 2, 3]
    ref_idx, ref_d = ranking.hamming_topk_stable(c["q"], c["r"], k)
    for f in forms:
        assert f[0].dtype == torch.int32 and f[1].dtype == torch.uint8 and tuple(f[0].shape) == tuple(f[1].shape) == (5, k)
        assert torch.equal(f[0], forms[0][0]) and torch.equal(f[1], forms[0][1])
    assert torch.equal(forms[0][0].cpu().long(), ref_idx) and torch.equal(forms[0][1].cpu().long(), ref_d)
    assert torch.equal(forms[3][2], c["cum"])
    assert H.hamming_topk(c["qp"], c["prep"], c["nbits"], k, want_dist=False)[1] is None


def test_hamming_topk_refuses_192_bit_codes_in_every_form():
    q, r = synth.random_codes(5, 700, 192, seed=192)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    prep = H.PreparedDB(rp, 192)
    for db, kw in ((rp, dict(workspace=H.TopkWorkspace())), (rp, {}), (prep, {}), (prep, dict(want_cum=True))):
        with pytest.raises(ValueError):
            H.hamming_topk(qp, db, 192, 37, **kw)


# ------------------------------------------------------------------------------------------------ virtual shards, lower edge
@pytest.fixture(scope="module")
def edge():
    """32,769 rows: two parts (16,385 + 16,384), 3 queries, 64-bit codes, 38 classes"""
    Q, N, nbits = 3, 32769, 64
    ql, rl = synth.multi_hot_labels(Q, 38, 0.1, 51), synth.multi_hot_labels(N, 38, 0.1, 52)
    q, r = synth.random_codes(Q, N, nbits, seed=53)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    prep, labels = H.PreparedDB(rp, nbits), H.PreparedLabels(rlp)
    assert len(prep.parts) == len(labels.parts) == 2 and [p.N for p in prep.parts] == [16385, 16384]
    idx, _ = H.hamming_topk(qp, prep, nbits, 100, want_dist=False)
    assert torch.equal(idx.cpu().long(), ranking.hamming_topk_stable(q, r, 100)[0])
    return dict(qp=qp, prep=prep, labels=labels, qlp=qlp, rlp=rlp, idx=idx,
                want={k: H.map_at_k(idx, qlp, rlp, k=k) for k in (1, 100)})


@pytest.mark.parametrize("k", [1, 100])
def test_fused_map_on_two_virtual_shards_equals_ranking_then_ap(edge, k):
    c = edge
    got = H.hamming_map_at_k(c["qp"], c["prep"], c["labels"], c["qlp"], 64, k)
    assert got is not None and tuple(got[0].shape) == (3,)
    assert torch.equal(got[1], c["want"][k][1]) and torch.equal(_bits(got[0]), _bits(c["want"][k][0]))
    if k == 100:                                                 # a condition on the inputs: the equality is not 0 == 0
        assert (got[1] > 0).all()


def test_fused_map_at_several_cutoffs_on_two_virtual_shards(edge):
    c = edge
    ks = [100, 1, 100]
    got = H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], 64, ks)
    assert got is not None and tuple(got[0].shape) == tuple(got[1].shape) == (3, 3)
    for i, k in enumerate(ks):
        assert torch.equal(got[1][:, i], c["want"][k][1]) and torch.equal(_bits(got[0][:, i]), _bits(c["want"][k][0])), k


# ------------------------------------------------------------------------------------------------ the refusal
def test_a_prefix_beyond_the_windowed_kernels_lists_is_refused_by_the_fused_map_only():
    """65,300 rows = two parts of 32,650, k = N: every part owes all its rows, 32,650 > RANK_K_MAX = 32,639 list entries.
    Both fused functions answer None (the caller ranks, then evaluates); hamming_topk ranks the same shape exactly."""
    Q, N, nbits = 2, 65300, 64
    ql, rl = synth.multi_hot_labels(Q, 38, 0.1, 61), synth.multi_hot_labels(N, 38, 0.1, 62)
    q, r = synth.random_codes(Q, N, nbits, seed=63)
    qp, prep = H.pack_codes(q.cuda()), H.PreparedDB(H.pack_codes(r.cuda()), nbits)
    qlp, labels = H.pack_labels(ql.cuda()), H.PreparedLabels(H.pack_labels(rl.cuda()))
    assert [p.N for p in prep.parts] == [32650, 32650] and labels.ok and prep.per > H.RANK_K_MAX
    assert H.hamming_map_at_k(qp, prep, labels, qlp, nbits, N) is None
    assert H.hamming_map_at_ks(qp, prep, labels, qlp, nbits, [N, 10]) is None
    idx, d = H.hamming_topk(qp, prep, nbits, N)
    ref_idx, ref_d = ranking.hamming_topk_stable(q, r, N)
    assert torch.equal(idx.cpu().long(), ref_idx) and torch.equal(d.cpu().long(), ref_d)
