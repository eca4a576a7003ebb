"""The dynamic LDS of the relevance-string merge (csrc/merge.hpp), as the library sizes it on the host (no GPU):
wv_merge_relbits_map_ks_lds_bytes sizes wv_merge_relbits_map and wv_merge_relbits_map_ks alike, and Python decides fallbacks
with it before any rank exchanges anything.  The figures follow from the layout: per shard nbits + 2 run boundaries of 4 bytes,
a string of k bits padded to 8 bytes (64 bits), and a part that depends on neither."""
import pytest

from wvhash.engine import hamming as H


@pytest.mark.parametrize("G,nbits", [(1, 64), (2, 64), (8, 128), (16, 33)])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000, 5000, 117218, 480001])
def test_the_string_costs_eight_bytes_per_64_bits(G, nbits, k):
    assert H.merge_relbits_lds_bytes(G, k + 64, nbits) - H.merge_relbits_lds_bytes(G, k, nbits) == 8


@pytest.mark.parametrize("G,nbits", [(1, 64), (2, 64), (8, 128), (16, 33), (3, 1)])
@pytest.mark.parametrize("k", [1, 100, 5000, 117218])
def test_a_shard_costs_its_run_boundaries(G, nbits, k):
    assert H.merge_relbits_lds_bytes(G + 1, k, nbits) - H.merge_relbits_lds_bytes(G, k, nbits) == 4 * (nbits + 2)


def test_the_limit_lies_between_the_shapes_that_fit_and_the_one_that_does_not():
    assert H.merge_relbits_lds_bytes(8, 117218, 128) <= H.MERGE_LDS_LIMIT < H.merge_relbits_lds_bytes(2, 2_000_000, 64)
    # any int is sized, not wrapped: the largest cut-off there is needs 2^26 + 1 words of string alone
    assert H.merge_relbits_lds_bytes(1, 2**31 - 1, 64) > 4 * 2**26


@pytest.mark.parametrize("G,k,nbits", [(0, 100, 64), (-1, 100, 64), (2, 0, 64), (2, -5, 64), (2, 100, 0), (2, 100, 129)])
def test_refused_arguments_size_to_zero(G, k, nbits):
    assert H.merge_relbits_lds_bytes(G, k, nbits) == 0
