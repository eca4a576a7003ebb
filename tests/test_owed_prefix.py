"""The prefix rule of the sharded Hamming search (wvhash.engine.hamming.owed_prefix) against brute force, on the CPU.

A query's global k-th distance T comes from the histograms summed over all shards; a shard owes the query its rows with
distance <= T.  Every route that sizes an exchange (virtual shards on one GPU, sharded_hamming_topk,
sharded_hamming_map_at_k) takes the rule from this one function, so it is pinned here on plain tensors: random +-1 codes,
three ragged parts, 8-bit codes (9 distinct distances: every cut falls inside a bucket of ties) and 64-bit codes.
"""
import pytest
import torch

from oracle import ranking
from wvhash import synth
from wvhash.engine import hamming as H

PARTS = ((0, 40), (40, 80), (80, 97))
Q = 7


@pytest.fixture(scope="module", params=[8, 64])
def shards(request):
    """-> (nbits, distance matrix [Q, 97], cumulative histograms [G, Q, nbits + 2] of the parts)"""
    nbits = request.param
    q, r = synth.random_codes(Q, PARTS[-1][1], nbits, seed=nbits)
    dm = ranking.hamming_matrix_u8(q, r).long()
    cum = torch.stack([torch.stack([(dm[:, lo:hi] < b).sum(1) for b in range(nbits + 2)], dim=1) for lo, hi in PARTS]).int()
    return nbits, dm, cum


@pytest.mark.parametrize("k", [1, 13, 97])
def test_owed_prefix_is_the_longest_run_of_rows_within_the_global_kth_distance(shards, k):
    nbits, dm, cum = shards
    T = dm.sort(dim=1).values[:, k - 1]                            # every query's k-th smallest distance over all rows
    want = max(int((dm[q, lo:hi] <= T[q]).sum()) for lo, hi in PARTS for q in range(Q))
    total = cum.sum(0)
    got = H.owed_prefix(cum, total, k)                             # all parts at once, their own sum
    assert got.dtype == torch.int32 and tuple(got.shape) == (1,) and int(got) == want
    # one shard at a time against the separate total (what a rank of the sharded search holds): the maximum is the same
    each = [H.owed_prefix(cum[g], total, k) for g in range(len(PARTS))]
    assert all(e.dtype == torch.int32 and tuple(e.shape) == (1,) for e in each)
    assert [int(e) for e in each] == [max(int((dm[q, lo:hi] <= T[q]).sum()) for q in range(Q)) for lo, hi in PARTS]
    assert max(int(e) for e in each) == want
    if k == PARTS[-1][1]:                                          # every row is owed: the longest part
        assert want == 40
