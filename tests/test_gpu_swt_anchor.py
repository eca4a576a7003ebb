"""GPU: the HIP SWT / DWT kernels against numbers the REFERENCE's own lifting code produced -- every row of the table of
tests/swt_anchor_cases.py (identities, fixed frames, bounds; the same float32 bounds as tests/test_swt_anchor.py holds the
host twins to) through

  * swt2d on the release library, on the kernel the restated planner names (sliding at 224^2, 64 x 96 and 64 x 48, tiled
    for bior4.4 level 2, generic at 40 x 30);
  * swt2d on the diagnostic library with WV_SWT_PATH pinned to each path that takes the row;
  * swt2d_band, band by band;
  * dwt2d at level 1.

Which kernel produced the numbers: wv_swt2d_workspace_bytes must equal what the restated planner says (only the generic
kernels need a workspace; the proof of tests/test_gpu_swt_fallback.py), and, layout by layout, the same call WITHOUT a
workspace must be refused with WV_ENOMEM exactly when the generic kernels are the ones to run -- that settles the one
combination the size alone leaves open (sliding path pinned, C != 3: the workspace is there for NHWC only).

Float32 NCHW input throughout, NHWC as well where a case has more than one plane; every output buffer is pre-filled with
NaN; only tests/golden/*.npz is read.  Every test prints the worst residual of its row."""
import ctypes

import numpy as np
import pytest
import torch

import swt_anchor_cases as A
import swt_fallback_cases as fc
from wvhash import _lib
from wvhash.transforms import get_filters, swt2d, swt2d_band

pytestmark = pytest.mark.gpu

ROW_IDS = [A.row_id(r) for r in A.ROWS]
DWT_IDS = [A.row_id(r) for r in A.DWT_ROWS]
WV_ENOMEM = -12


def nan_buffer(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def layouts(row):
    """-> [(name, GPU tensor, channels_last)]: NCHW, and NHWC when the case has more than one plane."""
    x = torch.from_numpy(A.case_input(row.file, row.case).copy())
    out = [("nchw", x.cuda(), False)]
    if x.shape[0] * x.shape[1] > 1:
        out.append(("nhwc", x.permute(0, 2, 3, 1).contiguous().cuda(), True))
    return out


def refused_without_workspace(x, cl, row):
    """wv_swt2d_forward on the current library with no workspace -> True when it is refused with WV_ENOMEM and nothing is
    written (the generic kernels were to run), False when it runs (another kernel did)."""
    lib = _lib.require_gpu()
    B, C, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if cl else x.shape
    lo, hi = get_filters(row.wavelet)
    out = nan_buffer((B, C, 4, H, W))
    rc = lib.wv_swt2d_forward(_lib.ptr(x), _lib.WV_DT_F32, _lib.WV_LAYOUT_NHWC if cl else _lib.WV_LAYOUT_NCHW, _lib.ptr(out),
                              _lib.WV_DT_F32, B, C, H, W, row.level, _lib.host_floats(lo), _lib.host_floats(hi), len(lo),
                              None, ctypes.c_size_t(0), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc in (0, WV_ENOMEM), (rc, lib.wv_last_error())
    assert bool(torch.isnan(out).all()) if rc else bool(torch.isfinite(out).all())
    return rc == WV_ENOMEM


def run_swt(row, pin):
    """The row through swt2d on the current library (pin = WV_SWT_PATH already set, or None), each layout on the kernel
    the restated planner names -> the worst residual."""
    N, C, H, W = A.case_input(row.file, row.case).shape
    L = fc.TAPS[row.wavelet]
    lib = _lib.require_gpu()
    assert (lib is _lib._DIAG) == bool(pin), "a pinned row needs the diag fixture, an unpinned one the release library"
    need = lib.wv_swt2d_workspace_bytes(N, C, H, W, row.level, L)
    assert need == fc.workspace_bytes(L, row.level, H, W, C, pin, batch=N), (A.row_id(row), pin, need)
    worst = 0.0
    for name, x, cl in layouts(row):
        path = fc.path(L, row.level, H, W, C, cl, pin)
        if pin and path != pin:
            continue                                                    # the pinned path does not take this layout
        assert refused_without_workspace(x, cl, row) == (path == "generic"), (A.row_id(row), pin, name, path)
        out = nan_buffer((N, C, 4, H, W))
        got = swt2d(x, row.wavelet, row.level, channels_last=cl, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        worst = max(worst, A.check_swt(f"swt2d {path}{' (pinned)' if pin else ''} {name}", row, out.cpu().numpy()))
    return worst


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_swt2d_release_library(row):
    N, C, H, W = A.case_input(row.file, row.case).shape
    assert fc.path(fc.TAPS[row.wavelet], row.level, H, W, C, False) == row.release_path
    run_swt(row, None)


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_swt2d_every_pinned_path_that_fits(row, diag):
    N, C, H, W = A.case_input(row.file, row.case).shape
    L = fc.TAPS[row.wavelet]
    pins = [p for p in A.PINS if fc.path(L, row.level, H, W, C, False, p) == p]
    assert "generic" in pins and row.release_path in pins
    for pin in pins:
        diag.setenv("WV_SWT_PATH", pin)
        run_swt(row, pin)


@pytest.mark.parametrize("row", A.ROWS, ids=ROW_IDS)
def test_swt2d_band_every_band(row):
    N, C, H, W = A.case_input(row.file, row.case).shape
    for name, x, cl in layouts(row):
        out = nan_buffer((N, C, 4, H, W))
        for band in range(4):
            one = nan_buffer((N, C, H, W))
            swt2d_band(x, row.wavelet, row.level, band, channels_last=cl, out=one)
            out[:, :, band] = one
        torch.cuda.synchronize()
        A.check_swt(f"swt2d_band {name}", row, out.cpu().numpy())


@pytest.mark.parametrize("row", A.DWT_ROWS, ids=DWT_IDS)
def test_dwt2d_level1(row):
    lib = _lib.require_gpu()
    N, C, H, W = A.case_input(row.file, row.case).shape
    lo, hi = get_filters(row.wavelet)
    Hn, Wn = lib.wv_dwt_out_len(H, len(lo), 1), lib.wv_dwt_out_len(W, len(lo), 1)
    need = lib.wv_dwt2d_workspace_bytes(N, C, H, W, 1, len(lo))
    for name, x, cl in layouts(row):
        out = nan_buffer((N, C, 4, Hn, Wn))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        rc = lib.wv_dwt2d_forward(_lib.ptr(x), _lib.WV_DT_F32, _lib.WV_LAYOUT_NHWC if cl else _lib.WV_LAYOUT_NCHW,
                                  _lib.ptr(out), N, C, H, W, 1, _lib.host_floats(lo), _lib.host_floats(hi), len(lo),
                                  _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream_ptr())
        assert rc == 0, lib.wv_last_error()
        torch.cuda.synchronize()
        A.check_dwt(f"dwt2d {name}", row, out.cpu().numpy())
