"""Host twins of the NDCG entry points (csrc/host_ndcg.cpp) on a GPU-less box: the overlap histogram against the bincount of
ql @ rl.T, exactly; DCG and ideal DCG against the numpy restatement of the definitions (tests/ndcg_cases.py) within the
derived tolerance; a multi-cut column against the single-cut call, bit for bit; arguments refused before any pointer is read
-- by the device entry points too, which need no GPU for that."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ndcg_cases as C
from wvhash import _lib
from wvhash.engine import hamming_host as HH
from wvhash.engine import ndcg as ND


def brute_hist(ql, rl):
    bins = 64 * ((ql.shape[1] + 63) // 64) + 1
    Rel = C.overlaps(ql.numpy(), rl.numpy())
    return np.stack([np.bincount(row, minlength=bins) for row in Rel])


@pytest.mark.parametrize("classes", C.HIST_CLASSES)
def test_overlap_hist_equals_bincount(classes):
    for N in C.HIST_N:
        for Q in C.HIST_Q:
            ql, rl = C.make_labels(Q, N, classes, min(0.5, 3.0 / classes), 7 * N + Q)
            hist = HH.label_overlap_hist(HH.pack_labels(ql), HH.pack_labels(rl))
            assert hist.dtype == torch.int32 and np.array_equal(hist.numpy(), brute_hist(ql, rl)), (classes, N, Q)
            assert int(hist[0, 0]) == N and int(hist[0].sum()) == N          # a query without classes: everything in bin 0


@pytest.mark.parametrize("classes", [38, 64, 128])
def test_overlap_hist_edges_and_shards(classes):
    N, Q = 1000, 7
    ql, rl = C.make_labels(Q, N, classes, 0.1, 3)
    full = 64 * ((classes + 63) // 64)
    if classes == full:                                        # query 1 and row 0 carry all 64 * lwords classes: the last bin
        h = HH.label_overlap_hist(HH.pack_labels(ql), HH.pack_labels(rl))
        assert int(h[1, full]) == 1 and h.shape[1] == full + 1
    same = ql[2:3].repeat(N, 1)                                # every row carries query 2's labels: one bin holds all N
    h = HH.label_overlap_hist(HH.pack_labels(ql), HH.pack_labels(same))
    assert int(h[2, int(ql[2].sum())]) == N
    qlp, rlp = HH.pack_labels(ql), HH.pack_labels(rl)
    whole = HH.label_overlap_hist(qlp, rlp)
    assert torch.equal(HH.label_overlap_hist(qlp, rlp[:333]) + HH.label_overlap_hist(qlp, rlp[333:]), whole)   # shards add up


@functools.lru_cache(maxsize=None)
def walk_inputs(classes, N=1200, Q=5):
    ql, rl = C.make_labels(Q, N, classes, min(0.5, 4.0 / classes), 11 + classes)
    ql[2] = 0                                                  # query 2 is lone like query 0 ...
    if classes in (38, 80):                                    # ... here through a class that no row carries
        ql[2, classes - 1] = 1
        rl[:, classes - 1] = 0
    else:                                                      # 60, 128: query 1 and row 0 share EVERY class (overlap 60 / 128)
        rl[3] = 0
        rl[3, :60] = 1                                         # and row 3 shares 60 with query 1
    idx = C.random_lists(Q, N, N, 5, absent=9)
    idx[:, 0] = torch.tensor([0, 0, 0, 3, 3])[:Q].int()        # the richest rows near the top
    return ql, rl, HH.pack_labels(ql), HH.pack_labels(rl), idx, C.overlaps(ql.numpy(), rl.numpy())


@pytest.mark.parametrize("classes", [38, 60, 80, 128])
def test_walk_against_the_restatement(classes):
    ql, rl, qlp, rlp, idx, Rel = walk_inputs(classes)
    N = rl.shape[0]
    assert Rel.max() == {38: 37, 60: 60, 80: 79, 128: 128}[classes] and (Rel[2] == 0).all() and (Rel[1] == 60).any() == (classes in (60, 128))
    for k in C.WALK_KS + [N]:
        dcg, idcg = HH.ndcg_at_ks(idx, qlp, rlp, [k])
        want_d, want_i = C.dcg_sums(idx.numpy(), Rel, k)
        C.assert_sums_close(dcg[:, 0].numpy(), want_d, k, "dcg")
        C.assert_sums_close(idcg[:, 0].numpy(), want_i, k, "idcg")
        assert float(dcg[2, 0]) == 0.0 and float(idcg[2, 0]) == 0.0                      # the lone query
        got = ND.ndcg_from_sums(dcg, idcg)
        assert torch.isfinite(got).all() and abs(float(got[0]) - C.ndcg_restated(idx.numpy(), Rel, k)) <= C.ndcg_tol(k)


@pytest.mark.parametrize("ks", [(255, 256, 257), (1, 2, 63, 64, 65, 128, 255, 256, 257, 300, 511, 512, 513, 800, 1000, 1200),
                                (100, 1000), (7,)])
def test_multi_cut_columns_have_the_bits_of_single_cut_calls(ks):
    ql, rl, qlp, rlp, idx, Rel = walk_inputs(80)
    wide = torch.full((idx.shape[0], idx.shape[1] + 37), -7, dtype=torch.int32)          # ld > k_max: a view with a pitch
    wide[:, :idx.shape[1]] = idx
    hist = HH.label_overlap_hist(qlp, rlp)
    dcg, idcg = HH.ndcg_at_ks(wide[:, :max(ks) + 5], qlp, rlp, list(ks), hist=hist)
    assert dcg.shape == (idx.shape[0], len(ks)) and dcg.dtype == torch.float64
    for i, k in enumerate(ks):
        d1, i1 = HH.ndcg_at_ks(idx, qlp, rlp, [k])
        assert torch.equal(dcg[:, i].view(torch.int64), d1[:, 0].view(torch.int64)), k
        assert torch.equal(idcg[:, i].view(torch.int64), i1[:, 0].view(torch.int64)), k
        C.assert_sums_close(dcg[:, i].numpy(), C.dcg_sums(idx.numpy(), Rel, k)[0], k, "dcg")
    back = HH.ndcg_at_ks(idx, qlp, rlp, list(reversed(ks)) + [ks[0]])[0]                  # any order, repeats: mapped back
    assert torch.equal(back[:, 0], dcg[:, -1]) and torch.equal(back[:, -1], dcg[:, 0])


def test_weights_are_reciprocal_logs():
    w = (ctypes.c_double * 5)()
    assert _lib.load().wv_ndcg_weights(w, 5) == 0
    assert list(w) == [1.0 / np.log2(p + 2.0) for p in range(5)] and w[0] == 1.0
    assert _lib.load().wv_ndcg_weights(None, 5) == -22 and _lib.load().wv_ndcg_weights(w, -1) == -22


def test_arguments_are_refused_before_any_pointer_is_read():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                  # never dereferenced: validation fails first
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    for cpu in (True, False):
        tail = () if cpu else (None,)
        hist = lib.wv_label_overlap_hist_cpu if cpu else lib.wv_label_overlap_hist
        walk = lib.wv_ndcg_at_ks_cpu if cpu else lib.wv_ndcg_at_ks
        assert hist(None, one, 1, 4, 100, one, *tail) == -22 and b"null buffer" in lib.wv_last_error()
        assert hist(one, one, 1, 4, 100, None, *tail) == -22
        assert hist(one, one, 3, 4, 100, one, *tail) == -95 and b"lwords=3" in lib.wv_last_error()
        assert hist(one, one, 0, 4, 100, one, *tail) == -95
        assert hist(one, one, 1, -1, 100, one, *tail) == -22
        assert hist(one, one, 2, 4, 0, one, *tail) == -22 and b"N=0" in lib.wv_last_error()
        assert hist(one, one, 2, 0, 100, one, *tail) == 0                                 # no queries: nothing to do
        call = lambda ks, nk, ld=100, lw=1, Q=4, p=one: walk(p, ld, Q, ks, nk, one, one, lw, one, one, one, one, *tail)
        assert call(ints(10), 1, p=None) == -22 and b"null buffer" in lib.wv_last_error()
        assert call(ints(10), 1, lw=3) == -95 and call(ints(10), 1, lw=0) == -95
        assert call(None, 1) == -22 and b"null cut-off list" in lib.wv_last_error()
        assert call(ints(10), 0) == -22 and call(ints(*range(1, 18)), 17) == -22 and b"17 cut-offs" in lib.wv_last_error()
        assert call(ints(0, 5), 2) == -22 and b"must be >= 1" in lib.wv_last_error()
        assert call(ints(5, 5), 2) == -22 and call(ints(7, 5), 2) == -22 and b"strictly ascending" in lib.wv_last_error()
        assert call(ints(5, 101), 2) == -22 and b"must be <= ld=100" in lib.wv_last_error()
        assert call(ints(5), 1, ld=0) == -22 and call(ints(5), 1, Q=-1) == -22
        assert call(ints(5, 100), 2, Q=0) == 0
    with pytest.raises(ValueError):
        HH.ndcg_at_ks(torch.zeros((2, 10), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64),
                      torch.zeros((5, 1), dtype=torch.int64), [11])
    with pytest.raises(ValueError):
        HH.label_overlap_hist(torch.zeros((2, 3), dtype=torch.int64), torch.zeros((5, 3), dtype=torch.int64))
