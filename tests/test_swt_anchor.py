"""CPU: every SWT / DWT implementation that runs without a GPU against numbers the REFERENCE's own lifting code produced
(tests/swt_anchor_cases.py holds the identities, the fixed frames and the bounds): the NumPy restatement in float64 and
float32, the C restatement, and the host twins of the library (four-band, single-band, DWT).  Every test prints the worst
residual of its row.

What this pins that nothing else does: the tap offset 2^(l-1) (L/2 - m), the axis order, cH = 'da', the sign of dec_hi
and the tap tables of haar (levels 1-3), db2 (levels 1-3) and bior4.4 (levels 1-2) -- in the oracle AND in the library's
own tables (wvhash/transforms/wavelets.py, which the twins read) -- and the level-1 DWT off its border."""
import numpy as np
import pytest
import torch

import swt_anchor_cases as A
import swt_fallback_cases as fc
from oracle import swt_np
from wvhash.transforms import dwt2d_host, swt2d_band_host, swt2d_host

ROW_IDS = [A.row_id(r) for r in A.ROWS]
DWT_IDS = [A.row_id(r) for r in A.DWT_ROWS]


def per_plane(x, fn):
    """fn([H, W]) -> [4, h, w] over every plane of x [N, C, H, W] -> [N, C, 4, h, w]."""
    return np.stack([np.stack([fn(x[b, c]) for c in range(x.shape[1])]) for b in range(x.shape[0])])


def test_fixtures_hold_what_the_table_needs():
    assert len({(r.file, r.case) for r in A.ROWS}) == 7 and len(A.ROWS) == 14 and len(A.DWT_ROWS) == 7
    g = A.gold("anchor")
    assert sorted({k.split("/")[0] for k in g.files}) == ["db2_224", "db2_40x30", "db2_64x96"]
    for case, shape, levels in (("db2_224", (1, 1, 224, 224), 3), ("db2_64x96", (1, 2, 64, 96), 2),
                                ("db2_40x30", (1, 2, 40, 30), 1)):
        assert tuple(g[f"{case}/shape"]) == shape
        assert len([k for k in g.files if k.startswith(case + "/l") and k.endswith("/ll")]) == levels
    for r in A.ROWS:
        want, x = A.expected(r), A.case_input(r.file, r.case)
        assert want.dtype == np.float32 and x.dtype == np.float32
        assert want.shape == x.shape[:2] + (4, x.shape[2] >> r.level, x.shape[3] >> r.level)
        assert r.level in A.OFFSET[r.wavelet] and r.level in A.FRAME[r.wavelet]


def test_release_paths_of_the_table_are_the_planners():
    """The kernel each row reaches on the release library, by the restated planner (swt_fallback_cases.path)."""
    for r in A.ROWS:
        _, C, H, W = A.case_input(r.file, r.case).shape
        assert fc.path(fc.TAPS[r.wavelet], r.level, H, W, C, False) == r.release_path, r
    assert {r.release_path for r in A.ROWS if r.case in ("db2_224", "db2_64x96", "haar_224")} == {"slide"}
    assert [r.release_path for r in A.ROWS if r.case == "db2_40x30"] == ["generic"]


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_numpy_oracle_fp64(row):
    x = A.case_input(row.file, row.case)
    A.check_swt("swt_np fp64", row, per_plane(x, lambda p: swt_np.swt2_level_n(p, row.wavelet, row.level, np.float64)), fp32=False)


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_numpy_oracle_fp32(row):
    x = A.case_input(row.file, row.case)
    A.check_swt("swt_np fp32", row, per_plane(x, lambda p: swt_np.swt2_level_n(p, row.wavelet, row.level, np.float32)))


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_c_oracle(row):
    x = A.case_input(row.file, row.case)
    A.check_swt("c oracle", row, per_plane(x, lambda p: swt_np.c_swt2_level_n(p, row.wavelet, row.level)))


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_host_twin(row):
    x = torch.from_numpy(A.case_input(row.file, row.case).copy())
    A.check_swt("swt2d_host", row, swt2d_host(x, row.wavelet, row.level).numpy())
    if x.shape[0] * x.shape[1] > 1:
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        A.check_swt("swt2d_host nhwc", row, swt2d_host(nhwc, row.wavelet, row.level, channels_last=True).numpy())


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_band_host_twin(row):
    x = torch.from_numpy(A.case_input(row.file, row.case).copy())
    y = torch.stack([swt2d_band_host(x, row.wavelet, row.level, band) for band in range(4)], dim=2)
    A.check_swt("swt2d_band_host", row, y.numpy())


@pytest.mark.parametrize("row", A.DWT_ROWS, ids=DWT_IDS)
def test_dwt_oracle_and_host_twin_level1(row):
    x = A.case_input(row.file, row.case)
    A.check_dwt("wavedec2 fp64", row, per_plane(x, lambda p: swt_np.wavedec2_coarsest(p, row.wavelet, 1, np.float64)), fp32=False)
    A.check_dwt("wavedec2 fp32", row, per_plane(x, lambda p: swt_np.wavedec2_coarsest(p, row.wavelet, 1, np.float32)))
    A.check_dwt("dwt2d_host", row, dwt2d_host(torch.from_numpy(x.copy()), row.wavelet, 1).numpy())


def test_a_wrong_shift_sign_or_pairing_is_far_above_the_bound():
    """The checks have teeth: on db2 level 3 a lattice one sample off, a flipped sign and swapped cH / cV each leave a
    residual more than four orders of magnitude above the bound."""
    row = next(r for r in A.ROWS if r.case == "db2_224" and r.level == 3)
    y = swt_np.swt2_level_n(A.case_input(row.file, row.case)[0, 0], "db2", 3, np.float64)[None, None]
    frame, want = A.FRAME["db2"][3], A.expected(row)
    lim = max(A.bounds(3, float(np.abs(A.case_input(row.file, row.case)).max()), True))
    for wrong in (np.roll(y, 1, axis=-1), np.roll(y, 1, axis=-2), -y, y[:, :, [0, 2, 1, 3]]):
        res = A.residuals(A.swt_to_lattice(wrong, "db2", 3), want, frame)
        assert max(res) > 1e4 * lim, (res, lim)
