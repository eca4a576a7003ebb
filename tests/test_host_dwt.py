"""CPU: the host twin of the decimated DWT (wv_dwt2d_forward_cpu, dwt2d_host) against the independent float64 reference
of tests/dwt_cases.py on the EDGE table -- every filter with every size shorter than it, one-pixel axes, levels past the
fixed point of n -> (n + F - 1) // 2 and the deepest level, both layouts, 1..4 channels, uint8 and float32 input -- under

    |twin - ref64|.max() <= 2 * |o32 - ref64|.max() + 2**-23 * |ref64|.max()

Worst err_twin / bound observed over the table: 0.571 (1.0 is the limit).
"""
import ctypes

import numpy as np
import pytest
import torch

import dwt_cases as D
from wvhash import _lib
from wvhash.transforms import dwt2d_host


@pytest.mark.parametrize("case", D.EDGE, ids=D.EDGE_IDS)
def test_twin_is_as_close_to_float64_as_the_float32_restatement(case):
    x, ref64, o32 = D.references(case.idx)
    before = x.copy()
    got = dwt2d_host(torch.from_numpy(x.copy()), D.TAPS[case.taps], case.level, channels_last=case.channels_last).numpy()
    assert got.dtype == np.float32 and got.shape == ref64.shape
    err, bound = D.error_and_bound(got, ref64, o32)
    print(f"{D.case_id(case)}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert np.isfinite(got).all() and err <= bound, (err, bound)
    assert np.array_equal(x, before)


def test_out_len_is_the_references_shape():
    lib = _lib.load()
    for F in (2, 3, 4, 5, 8, 10, 20, 32):
        f = np.ones(F)
        for n in list(range(1, 24)) + [37, 64]:
            a = np.zeros((n, 1))
            for level in (1, 2, 3, 6, 12):
                a = np.zeros((n, 1))
                for _ in range(level):
                    a = D.ref_axis(a, f, 0)
                assert lib.wv_dwt_out_len(n, F, level) == a.shape[0] == D.out_len(n, F, level), (F, n, level)


def test_workspace_bytes_is_zero_for_an_empty_problem():
    lib = _lib.load()
    assert lib.wv_dwt2d_workspace_bytes(2, 3, 37, 51, 2, 8) > 0
    for args in [(0, 3, 8, 8, 1, 2), (1, 0, 8, 8, 1, 2), (1, 3, 0, 8, 1, 2), (1, 3, 8, 0, 1, 2), (-1, 3, 8, 8, 1, 2),
                 (1, 3, 8, -8, 1, 2), (1, 3, 8, 8, 0, 2), (1, 3, 8, 8, -1, 2)]:
        assert lib.wv_dwt2d_workspace_bytes(*args) == 0, args


def test_twin_error_codes():
    lib = _lib.load()
    x = torch.zeros((1, 1, 8, 8), dtype=torch.uint8)
    o = torch.full((4 * 31 * 31,), -3.0)                         # room for the largest accepted call below (32 taps: 30 x 30)
    f = _lib.host_floats([0.5] * 33)

    def call(dtype=_lib.WV_DT_U8, layout=_lib.WV_LAYOUT_NCHW, level=1, taps=2):
        return lib.wv_dwt2d_forward_cpu(_lib.ptr(x), dtype, layout, _lib.ptr(o), 1, 1, 8, 8, level, f, f, taps)

    assert call(level=0) == -22 and call(level=13) == -22
    assert call(taps=1) == -22 and call(taps=33) == -22
    assert call(dtype=2) == -22
    assert call(layout=7) == -22
    assert bool((o == -3.0).all())
    assert call() == 0 and call(level=12, taps=32) == 0          # the same call with arguments in range goes through


def test_empty_batch_returns_the_empty_shape():
    for channels_last, shape in ((False, (0, 3, 37, 51)), (True, (0, 37, 51, 3))):
        y = dwt2d_host(torch.zeros(shape, dtype=torch.uint8), "db4", 2, channels_last=channels_last)
        assert tuple(y.shape) == (0, 3, 4, D.out_len(37, 8, 2), D.out_len(51, 8, 2)) and y.dtype == torch.float32
