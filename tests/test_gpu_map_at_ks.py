"""Average precision at several cut-offs from ONE ranking pass (wv_hamming_map_at_ks, wv_merge_relbits_map_ks, wv_map_at_ks)
against the single-k entry points, cut-off by cut-off.

The contract: column i has the BITS the single-k entry point returns for k = ks[i] (AP float32 compared through its int32
view, nrel exactly) whenever both run the same kernel variant -- always on the 256-thread ranking kernel, the merge kernel
and the list kernel; one wave per query sums in its own order and is compared with its own single-k runs (WV_TOPK_V2=64
pinned for both).  Inputs are seeded: labels Bernoulli(0.10) over 38 classes with at least one tag per row, so
two rows share a tag with probability ~0.32 and a query without a hit among 64 entries has probability 0.68^64 < 1e-10 --
asserted as a condition on the inputs, so that equality is never 0 == 0."""
import ctypes

import pytest
import torch

from oracle import ranking
from wvhash import _lib, synth
from wvhash.engine import hamming as H
from wvhash.engine import hamming_host as HH

pytestmark = pytest.mark.gpu

ORACLE_TOL = 6e-8            # AP against the canonical oracle
KS_256 = (1, 255, 256, 257, 5000, 8192, 8193, 9000)     # round boundary 256, chunk boundary 32 * 256 = 8192, k_max = N
KS_64 = (1, 63, 64, 65, 1024, 2047, 2048)               # round boundary 64, chunk boundary 32 * 64 = 2048 = k_max


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(Q, N, nbits, classes, seed):
    ql, rl = synth.multi_hot_labels(Q, classes, 0.10, seed), synth.multi_hot_labels(N, classes, 0.10, seed + 1)
    q, r = synth.random_codes(Q, N, nbits, seed=Q + N + nbits)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    return dict(q=q, r=r, ql=ql, rl=rl, qp=qp, rp=rp, qlp=qlp, rlp=rlp, nbits=nbits, prep=H.PreparedDB(rp, nbits),
                labels=H.PreparedLabels(rlp))


@pytest.fixture(scope="module")
def c64():
    return _inputs(24, 9000, 64, 38, 1)


@pytest.fixture(scope="module")
def c128():
    return _inputs(24, 9000, 128, 80, 3)


def _assert_columns_equal_single_k(c, ks, got):
    ap, nrel = got
    assert tuple(ap.shape) == (c["qp"].shape[0], len(ks)) and ap.dtype == torch.float32 and nrel.dtype == torch.int32
    for i, k in enumerate(ks):
        one = H.hamming_map_at_k(c["qp"], c["prep"], c["labels"], c["qlp"], c["nbits"], k)
        assert one is not None, k
        assert torch.equal(nrel[:, i], one[1]), (k, nrel[:, i].tolist(), one[1].tolist())
        assert torch.equal(_bits(ap[:, i]), _bits(one[0])), (k, (ap[:, i] - one[0]).abs().max().item())
        if k >= 64:                                              # a condition on the inputs, not a tolerance
            assert (one[1] > 0).float().mean().item() >= 0.9, k


@pytest.mark.parametrize("case", ["c64", "c128"])
def test_256_thread_kernel_every_column_has_the_single_k_bits(case, request):
    """N = 9,000 rows, 24 queries: 64-bit codes with 38 classes (one label word), 128-bit codes with 80 classes (two)."""
    c = request.getfixturevalue(case)
    assert c["qlp"].shape[1] == (1 if case == "c64" else 2)
    got = H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], c["nbits"], KS_256)
    assert got is not None
    _assert_columns_equal_single_k(c, KS_256, got)


def test_one_wave_per_query_against_its_own_single_k_runs(diag):
    diag.setenv("WV_TOPK_V2", "64")
    c = _inputs(16, 3000, 64, 38, 5)
    got = H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], c["nbits"], KS_64)
    assert got is not None
    _assert_columns_equal_single_k(c, KS_64, got)


@pytest.mark.parametrize("variant", [None, "64"])
def test_cuts_inside_distance_buckets_and_around_window_slides(diag, variant):
    """8-bit codes: 9 distances for 9,000 rows, every cut lies inside a bucket of ~hundreds of ties.  128-bit rows that are
    the query with d = 0 .. 127 flipped bits, 20 rows per distance: a window holds 32 distances = 640 rows, so a list of
    1,500 entries makes the window slide twice; cuts before (100, 640), inside (641 .. 1281) and after (1500) the slides."""
    if variant is not None:
        diag.setenv("WV_TOPK_V2", variant)
    c = _inputs(24, 9000 if variant is None else 3000, 8, 38, 7)
    ks = (1, 100, 256, 1000, 2047, 2048) + ((4500, 8193, 9000) if variant is None else ())
    got = H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], 8, ks)
    assert got is not None
    _assert_columns_equal_single_k(c, ks, got)
    # the sliding window
    N, nbits = 2560, 128
    g = torch.Generator().manual_seed(11)
    q0 = torch.randint(0, 2, (nbits,), generator=g).float() * 2 - 1
    r = q0.repeat(N, 1)
    for i in range(N):
        flip = torch.randperm(nbits, generator=g)[:i % 128]
        r[i, flip] *= -1
    q = torch.stack([q0, -q0, torch.randint(0, 2, (nbits,), generator=g).float() * 2 - 1])
    d0 = ranking.hamming_matrix_u8(q[:1], r)[0]
    assert torch.equal(torch.bincount(d0, minlength=128), torch.full((128,), 20))
    ql, rl = synth.multi_hot_labels(3, 38, 0.10, 12), synth.multi_hot_labels(N, 38, 0.10, 13)
    rp, rlp = H.pack_codes(r.cuda()), H.pack_labels(rl.cuda())
    s = dict(qp=H.pack_codes(q.cuda()), qlp=H.pack_labels(ql.cuda()), nbits=nbits, prep=H.PreparedDB(rp, nbits),
             labels=H.PreparedLabels(rlp))
    ks = (100, 640, 641, 1000, 1280, 1281, 1500)
    got = H.hamming_map_at_ks(s["qp"], s["prep"], s["labels"], s["qlp"], nbits, ks)
    assert got is not None
    _assert_columns_equal_single_k(s, ks, got)
    idx, _ = H.hamming_topk(s["qp"], rp, nbits, 1500, want_dist=False)            # and against ranking + list kernel
    lst = H.map_at_ks(idx, s["qlp"], rlp, ks)
    assert torch.equal(got[1], lst[1])
    if variant is None:
        assert torch.equal(_bits(got[0]), _bits(lst[0]))


def test_virtual_shards_beyond_32768_rows():
    c = _inputs(16, 40000, 128, 80, 9)
    assert c["prep"].parts and len(c["prep"].parts) == 2
    ks = (100, 5000, 20001, 40000)
    got = H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], 128, ks)
    assert got is not None
    _assert_columns_equal_single_k(c, ks, got)


@pytest.mark.parametrize("short", [False, True])
def test_merge_of_relevance_strings_at_several_cutoffs(short):
    """G = 3 shards of 1,000, 1,000 and 700 rows.  The prefix length is chosen above what the largest cut needs (exact) and
    below it (flagged through need_out): either way the merged string is the single-k call's at k_max, so every column equals
    the single-k call on the same wires, and need_out is its value at k_max."""
    c = _inputs(19, 2700, 64, 38, 21)
    ks = (1, 50, 256, 257, 999, 1500)
    bounds = ((0, 1000), (1000, 2000), (2000, 2700))
    parts = [(H.PreparedDB(c["rp"][lo:hi].contiguous(), 64), H.PreparedLabels(c["rlp"][lo:hi].contiguous())) for lo, hi in bounds]
    cums = torch.stack([H.hamming_hist(c["qp"], db, 64) for db, _ in parts])
    need = int(H.owed_prefix(cums, cums.sum(0), ks[-1]).item())
    assert 2 <= need < 1000
    kin = need // 2 if short else need + 37
    wires = torch.zeros((3, 19, H.relbits_wire_words(kin, 64)), dtype=torch.int64, device="cuda")
    for g, (db, lab) in enumerate(parts):
        assert H.hamming_shard_relbits(c["qp"], db, lab, c["qlp"], 64, min(kin, db.N), wire=wires[g], kin=kin) is not None
    owed = torch.zeros(1, dtype=torch.int32, device="cuda")
    ap, nrel = H.merge_relbits_map_ks(wires, kin, ks, 64, need_out=owed)
    owed1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    H.merge_relbits_map(wires, kin, ks[-1], 64, need_out=owed1)
    assert int(owed.item()) == int(owed1.item()) == need and (need <= kin) == (not short)
    for i, k in enumerate(ks):
        ap1, nrel1 = H.merge_relbits_map(wires, kin, k, 64)
        assert torch.equal(nrel[:, i], nrel1) and torch.equal(_bits(ap[:, i]), _bits(ap1)), k
    if not short:                                                # exact exchange: the unsharded numbers
        _assert_columns_equal_single_k(c, ks, (ap, nrel))


@pytest.mark.parametrize("classes", [38, 80, 130])
def test_list_kernel_reads_the_lists_once_for_all_cutoffs(classes):
    """wv_map_at_ks over lists of pitch ld > k_max against wv_map_at_k_ld per cut-off and against the host twin (one, two and
    three label words: the last takes the kernels' generic label loop).  Both kernels live in list_ap.hip and share the
    relevance test, so the single-cut one is anchored to the host twin's own plain loop (wv_map_at_k_cpu), bit for bit, at
    every cut-off: 256 is the round boundary, 32 * 256 = 8192 the chunk boundary of the multi-cut walk."""
    c = _inputs(24, 9000, 64, classes, 31)
    idx, _ = H.hamming_topk(c["qp"], c["rp"], 64, 8500, want_dist=False)
    idx[5, 77] = -1                                              # an absent entry is skipped
    ks = (1, 255, 256, 257, 2048, 2049, 2500, 8191, 8192, 8193)
    assert idx.stride(0) == 8500 > ks[-1]
    idx_h, qlp_h, rlp_h = idx.cpu(), c["qlp"].cpu(), c["rlp"].cpu()
    ap, nrel = H.map_at_ks(idx, c["qlp"], c["rlp"], ks)
    for i, k in enumerate(ks):
        ap1, nrel1 = H.map_at_k(idx, c["qlp"], c["rlp"], k=k)
        assert torch.equal(nrel[:, i], nrel1) and torch.equal(_bits(ap[:, i]), _bits(ap1)), k
        ap1_h, nrel1_h = HH.map_at_k(idx_h, qlp_h, rlp_h, k=k)
        if k >= 64:                                              # a condition on the inputs, from the host twin alone
            assert (nrel1_h > 0).float().mean().item() >= 0.9
        assert torch.equal(nrel1.cpu(), nrel1_h), (k, nrel1.tolist(), nrel1_h.tolist())
        assert torch.equal(_bits(ap1.cpu()), _bits(ap1_h)), (k, (ap1.cpu() - ap1_h).abs().max().item())
    ap_h, nrel_h = HH.map_at_ks(idx_h, qlp_h, rlp_h, ks)
    assert torch.equal(nrel.cpu(), nrel_h) and torch.equal(_bits(ap.cpu()), _bits(ap_h))
    # the C entry point itself, nrel = NULL: the same AP bits, nothing else asked for
    k = 8193
    ap_c = torch.full((24,), float("nan"), device="cuda")
    with torch.cuda.device(idx.device):
        rc = _lib.load().wv_map_at_k_ld(_lib.ptr(idx), idx.stride(0), 24, k, _lib.ptr(c["qlp"]), _lib.ptr(c["rlp"]), c["qlp"].shape[1],
                                        _lib.ptr(ap_c), None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(_bits(ap_c.cpu()), _bits(HH.map_at_k(idx_h, qlp_h, rlp_h, k=k)[0]))


def test_against_the_oracles_canonical_order(c64, capsys):
    got = H.hamming_map_at_ks(c64["qp"], c64["prep"], c64["labels"], c64["qlp"], 64, KS_256)
    worst = 0.0
    for i, k in enumerate(KS_256):
        _, want = ranking.calculate_maphashing(c64["q"][:8], c64["ql"][:8], c64["r"], c64["rl"], k, stable=True, return_per_query=True)
        err = (got[0][:8, i].double().cpu() - torch.tensor(want, dtype=torch.float64)).abs().max().item()
        with capsys.disabled():
            print(f"\n  oracle AP@{k}: max |diff| = {err:.3e}", end="")
        worst = max(worst, err)
    assert worst <= ORACLE_TOL, worst


def test_cutoffs_arrive_unsorted_and_repeated_and_rows_follow_the_queries(c64):
    ks = (5000, 1, 9000, 5000, 256)
    got = H.hamming_map_at_ks(c64["qp"], c64["prep"], c64["labels"], c64["qlp"], 64, ks)
    _assert_columns_equal_single_k(c64, ks, got)
    perm = torch.randperm(24, generator=torch.Generator().manual_seed(3)).cuda()
    moved = H.hamming_map_at_ks(c64["qp"][perm].contiguous(), c64["prep"], c64["labels"], c64["qlp"][perm].contiguous(), 64, ks)
    assert torch.equal(_bits(moved[0]), _bits(got[0][perm])) and torch.equal(moved[1], got[1][perm])


def _c_call(c, ks, ap, nrel, N=None):
    lib = _lib.load()
    arr = (ctypes.c_int * max(len(ks), 1))(*ks)
    with torch.cuda.device(c["qp"].device):
        rc = lib.wv_hamming_map_at_ks(_lib.ptr(c["qp"]), _lib.ptr(c["prep"].blob), _lib.ptr(c["labels"].blob), _lib.ptr(c["qlp"]),
                                      c["qlp"].shape[1], c["qp"].shape[0], c["prep"].N if N is None else N, c["nbits"], arr, len(ks),
                                      _lib.ptr(ap), _lib.ptr(nrel), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_nothing_is_written_past_the_rows_and_old_content_does_not_matter(c64):
    Q, ks = 24, [1, 257, 8193]
    want = H.hamming_map_at_ks(c64["qp"], c64["prep"], c64["labels"], c64["qlp"], 64, ks)
    for fill in (0.0, float("nan")):
        ap = torch.full((Q * len(ks) + 64,), fill, device="cuda")
        nrel = torch.full((Q * len(ks) + 64,), -7, dtype=torch.int32, device="cuda")
        ap[Q * len(ks):] = -7.0
        assert _c_call(c64, ks, ap, nrel) == 0
        assert (ap[Q * len(ks):] == -7.0).all() and (nrel[Q * len(ks):] == -7).all()
        assert torch.equal(_bits(ap[:Q * len(ks)].view(Q, -1)), _bits(want[0]))
        assert torch.equal(nrel[:Q * len(ks)].view(Q, -1), want[1])
    ap = torch.empty((Q, len(ks)), device="cuda")                # nrel may be NULL
    assert _c_call(c64, ks, ap, None) == 0 and torch.equal(_bits(ap), _bits(want[0]))


def test_refusals_come_from_the_host_before_any_launch(c64):
    guard_a = torch.full((24, 17), -3.0, device="cuda")
    guard_n = torch.full((24, 17), -3, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    for bad in ([], list(range(1, 18)), [9, 4], [5, 5], [0, 4], [4, 9001]):
        assert _c_call(c64, bad, guard_a, guard_n) == -22, bad
        assert lib.wv_last_error()
    idx, _ = H.hamming_topk(c64["qp"], c64["rp"], 64, 100, want_dist=False)
    for bad in ([], list(range(1, 18)), [9, 4], [5, 5], [4, 101]):
        arr = (ctypes.c_int * max(len(bad), 1))(*bad)
        assert lib.wv_map_at_ks(_lib.ptr(idx), 100, 24, arr, len(bad), _lib.ptr(c64["qlp"]), _lib.ptr(c64["rlp"]), 1, _lib.ptr(guard_a),
                                _lib.ptr(guard_n), _lib.stream_ptr()) == -22, bad
        wire = torch.zeros((1, 24, H.relbits_wire_words(64, 64)), dtype=torch.int64, device="cuda")
        if bad != [4, 101]:
            assert lib.wv_merge_relbits_map_ks(wire.data_ptr() + 8 * 33, wire.shape[2], wire.data_ptr(), 2 * wire.shape[2], 1, 24, 64,
                                               arr, len(bad), 64, _lib.ptr(guard_a), _lib.ptr(guard_n), None, _lib.stream_ptr()) == -22, bad
    torch.cuda.synchronize()
    assert (guard_a == -3.0).all() and (guard_n == -3).all()
    with pytest.raises(ValueError):
        H.hamming_map_at_ks(c64["qp"], c64["prep"], c64["labels"], c64["qlp"], 64, list(range(1, 18)))
    with pytest.raises(ValueError):
        H.hamming_map_at_ks(c64["qp"], c64["prep"], c64["labels"], c64["qlp"], 64, [10, 9001])


def test_a_largest_cutoff_that_does_not_fit_is_refused_and_the_fallback_gives_the_same_numbers():
    """32,700 rows are inside one launch, a list of 32,700 entries is not (16-bit cells: k <= 32,639): WV_ENOTSUP with a sentence
    that says so, None in Python; ranking at k_max + wv_map_at_ks then gives, for the cut-offs the fused kernel does take, its
    numbers.  Likewise a merged string beyond the merge kernel's LDS."""
    c = _inputs(5, 32700, 64, 38, 41)
    ks = [100, 5000, 32700]
    ap = torch.full((5, 3), -3.0, device="cuda")
    nrel = torch.full((5, 3), -3, dtype=torch.int32, device="cuda")
    assert _c_call(c, ks, ap, nrel) == _lib.WV_ENOTSUP
    msg = _lib.load().wv_last_error().decode()
    assert "32700" in msg and "wv_map_at_ks" in msg, msg
    assert (ap == -3.0).all() and (nrel == -3).all()
    assert H.hamming_map_at_ks(c["qp"], c["prep"], c["labels"], c["qlp"], 64, ks) is None
    idx, _ = H.hamming_topk(c["qp"], c["prep"], 64, ks[-1], want_dist=False)
    fb_ap, fb_nrel = H.map_at_ks(idx, c["qlp"], c["rlp"], ks)
    for i, k in enumerate(ks):
        one = H.hamming_map_at_k(c["qp"], c["prep"], c["labels"], c["qlp"], 64, k)
        if one is None:
            assert k == 32700
            one = H.map_at_k(idx, c["qlp"], c["rlp"], k=k)
        assert torch.equal(fb_nrel[:, i], one[1]) and torch.equal(_bits(fb_ap[:, i]), _bits(one[0])), k
    # the merge: a 2,000,000-bit string does not fit 60 KB of LDS
    wire = torch.zeros((2, 5, H.relbits_wire_words(64, 64)), dtype=torch.int64, device="cuda")
    assert H.merge_relbits_map_ks(wire, 64, [10, 2000000], 64) is None
    assert "does not fit" in _lib.load().wv_last_error().decode()
    assert H.merge_relbits_lds_bytes(2, 2000000, 64) > H.MERGE_LDS_LIMIT >= H.merge_relbits_lds_bytes(8, 117218, 128)
    # the size Python decides fallbacks with is the entry point's own: the call flips to WV_ENOTSUP exactly where it crosses the limit
    fits = max(k for k in range(475000, 490000, 32) if H.merge_relbits_lds_bytes(2, k, 64) <= H.MERGE_LDS_LIMIT)
    assert H.merge_relbits_lds_bytes(2, fits + 32, 64) > H.MERGE_LDS_LIMIT
    assert H.merge_relbits_map_ks(wire, 64, [10, fits], 64) is not None
    assert H.merge_relbits_map_ks(wire, 64, [10, fits + 32], 64) is None
    # a single cut-off keeps the same string in the same LDS layout: the same refusal, the same sentence, the same flip
    assert H.merge_relbits_map(wire, 64, 2000000, 64) is None
    assert "does not fit" in _lib.load().wv_last_error().decode()
    assert H.merge_relbits_map(wire, 64, fits, 64) is not None
    assert H.merge_relbits_map(wire, 64, fits + 32, 64) is None
    ap = torch.full((5,), -3.0, device="cuda")
    nrel = torch.full((5,), -3, dtype=torch.int32, device="cuda")
    with torch.cuda.device(wire.device):
        rc = _lib.load().wv_merge_relbits_map(wire.data_ptr() + 8 * 33, wire.shape[2], wire.data_ptr(), 2 * wire.shape[2], 2, 5, 64,
                                              2000000, 64, _lib.ptr(ap), _lib.ptr(nrel), None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.WV_ENOTSUP and (ap == -3.0).all() and (nrel == -3).all()
