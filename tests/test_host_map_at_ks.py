"""Average precision at several cut-offs from one walk, host side (no GPU): wv_map_at_ks_cpu against wv_map_at_k_cpu per cut-off
-- bit for bit: a thread's quotients are added in increasing list position, so the state after position c - 1 is the state of
a walk to c --, CustomCalculator(device='cpu').calculate_maphashing_at against its per-k calculate_maphashing, and the four new
symbols in the header and in both libraries."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from wvhash import _lib, synth
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming_host as HH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wv_hamming_map_at_ks", "wv_merge_relbits_map_ks", "wv_map_at_ks", "wv_map_at_ks_cpu")


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ranked():
    """Labels Bernoulli(0.10) over 38 classes, at least one tag per row (two rows share a tag with probability ~0.32);
    lists of 3000 entries out of 3100 rows with pitch 3000, one entry marked absent (< 0)."""
    Q, N, nbits, k = 9, 3100, 64, 3000
    ql, rl = synth.multi_hot_labels(Q, 38, 0.10, 1), synth.multi_hot_labels(N, 38, 0.10, 2)
    q, r = synth.random_codes(Q, N, nbits, seed=Q + N)
    idx, _ = HH.hamming_topk(HH.pack_codes(q), HH.pack_codes(r), nbits, k)
    idx[3, 700] = -1
    return idx, HH.pack_labels(ql), HH.pack_labels(rl), (q, ql, r, rl)


# round boundaries (256), chunk boundaries (32 rounds x 256 would be 8192: beyond these lists; 2048 = 8 rounds), the list's end
KS = (1, 2, 255, 256, 257, 511, 512, 1000, 2047, 2048, 2049, 2999, 3000)


def test_host_twin_equals_single_k_twin_bit_for_bit(ranked):
    idx, qlp, rlp, _ = ranked
    ap, nrel = HH.map_at_ks(idx, qlp, rlp, KS)
    assert tuple(ap.shape) == (idx.shape[0], len(KS)) and ap.dtype == torch.float32 and nrel.dtype == torch.int32
    for i, k in enumerate(KS):
        ap1, nrel1 = HH.map_at_k(idx, qlp, rlp, k=k)
        assert torch.equal(_bits(ap[:, i]), _bits(ap1)), k
        assert torch.equal(nrel[:, i], nrel1), k
    for k in KS:                                                 # a condition on the inputs: equality is not 0 == 0
        if k >= 64:
            assert (HH.map_at_k(idx, qlp, rlp, k=k)[1] > 0).float().mean() >= 0.9


def test_cutoffs_unsorted_and_repeated_map_back_to_their_columns(ranked):
    idx, qlp, rlp, _ = ranked
    ks = (2048, 5, 2048, 1, 3000, 5)
    ap, nrel = HH.map_at_ks(idx, qlp, rlp, ks)
    for i, k in enumerate(ks):
        ap1, nrel1 = HH.map_at_k(idx, qlp, rlp, k=k)
        assert torch.equal(_bits(ap[:, i]), _bits(ap1)) and torch.equal(nrel[:, i], nrel1)


def test_c_entry_point_checks_and_writes_only_its_columns(ranked):
    idx, qlp, rlp, _ = ranked
    lib = _lib.load()
    Q, ld = idx.shape

    def call(ks, ap, nrel):
        arr = (ctypes.c_int * max(len(ks), 1))(*ks)
        return lib.wv_map_at_ks_cpu(_lib.ptr(idx), ld, Q, arr, len(ks), _lib.ptr(qlp), _lib.ptr(rlp), qlp.shape[1], _lib.ptr(ap),
                                    _lib.ptr(nrel))
    ks = [7, 300, 2900]
    ap = torch.full((Q, len(ks) + 1), -7.0)                      # one guard column behind the rows ...
    nrel = torch.full((Q, len(ks) + 1), -7, dtype=torch.int32)
    # ... which the call must treat as the next row's first entries: pass a tight [Q][nk] buffer inside a larger one
    ap_t, nrel_t = ap.view(-1)[:Q * len(ks)], nrel.view(-1)[:Q * len(ks)]
    assert call(ks, ap_t, nrel_t) == 0
    assert (ap.view(-1)[Q * len(ks):] == -7.0).all() and (nrel.view(-1)[Q * len(ks):] == -7).all()
    want = HH.map_at_ks(idx, qlp, rlp, ks)
    assert torch.equal(_bits(ap_t.view(Q, -1)), _bits(want[0])) and torch.equal(nrel_t.view(Q, -1), want[1])
    # results do not depend on what the outputs held; nrel may be NULL
    ap2 = torch.full((Q, len(ks)), float("nan"))
    arr = (ctypes.c_int * 3)(*ks)
    assert lib.wv_map_at_ks_cpu(_lib.ptr(idx), ld, Q, arr, 3, _lib.ptr(qlp), _lib.ptr(rlp), qlp.shape[1], _lib.ptr(ap2), None) == 0
    assert torch.equal(_bits(ap2), _bits(want[0]))
    # refusals: WV_EINVAL, outputs untouched
    guard_a, guard_n = torch.full((Q, 17), -3.0), torch.full((Q, 17), -3, dtype=torch.int32)
    for bad in ([], list(range(1, 18)), [5, 5], [9, 4], [0, 4], [4, ld + 1]):
        assert call(bad, guard_a, guard_n) == -22, bad
        assert lib.wv_last_error()
    assert (guard_a == -3.0).all() and (guard_n == -3).all()
    with pytest.raises(ValueError):
        HH.map_at_ks(idx, qlp, rlp, list(range(1, 18)))
    with pytest.raises(ValueError):
        HH.map_at_ks(idx, qlp, rlp, [ld + 1])


def test_cpu_calculator_answers_every_cutoff_like_its_single_k_form(ranked):
    _, _, _, (q, ql, r, rl) = ranked
    calc = CustomCalculator(k=100, device="cpu", distance_metric="hamming", with_faiss=False)
    ks = [100, 1, 3100, 257, 5000, 100]                          # 5000 > N clips at N like gnd[0:topk]
    got = calc.calculate_maphashing_at(q, ql, r, rl, ks)
    assert list(got) == [100, 1, 3100, 257, 5000]
    for k in ks:
        assert got[k] == calc.calculate_maphashing(q, ql, r, rl, k), k
    per = calc.calculate_maphashing_at(q, ql, r, rl, [257], return_per_query=True)[257]
    value, ap = calc.calculate_maphashing(q, ql, r, rl, 257, return_per_query=True)
    assert per[0] == value and torch.equal(_bits(per[1]), _bits(ap))
    assert "maphashing_at" not in calc.get_curr_metrics()        # a method with cut-offs of its own, not a get_accuracy column
    with pytest.raises(ValueError):
        calc.calculate_maphashing_at(q, ql, r, rl, [])


def test_header_declares_and_both_libraries_export_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "wvhash.h")).read()
    assert re.search(r"#define\s+WV_MAX_CUTOFFS\s+16\b", header)
    assert re.search(r"#define\s+WV_ABI_VERSION\s+5\b", header) or _lib.ABI_VERSION == 5
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for sym in NEW_SYMBOLS:
            assert re.search(rf"\bint\s+{sym}\s*\(", header), sym
            assert sym in _lib.SIGNATURES, sym
            assert re.search(rf"\sT\s+{sym}$", exported, re.M), (path, sym)
    assert _lib.load().wv_abi_version() == 5
