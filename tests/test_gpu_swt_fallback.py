"""The three SWT implementations behind the sliding kernel -- register-fused (csrc/swt_fused.hip), tiled and generic
(csrc/swt.hip) -- at their tile edges, every template instantiation launched by an asserted case.

Instantiations, and the rule that produces the counts:
  fused   32 = 8 (taps, level) of WV_SWT_CONFIGS x {u8, f32} input x {wide TW = 112, narrow TW = 64} tile (pick_shape); the
          output type and the input layout are run-time branches of each.
  tiled   48 = 12 (taps, level), taps 2 / 4 / 8 / 10 x levels 1-3, x {u8, f32} input x {f32, bf16} output; the layout is a
          run-time branch.
  generic k_planes_to_f32 x {u8, f32} and k_axis_generic x {f32, bf16}.
The tables (tests/swt_fallback_cases.py; what each row is there for is asserted without a GPU by
tests/test_swt_fallback_cases.py) run all four input forms {u8, f32} x {NCHW, NHWC} and both output types on every row of
the pinned fused and tiled tables, so each of the 32 + 48 kernels runs at a shape with partial tiles.

Which kernel produced the numbers: WV_SWT_PATH (diagnostic library) pins a path, but a pinned path that does not fit turns
into generic silently.  wv_swt2d_workspace_bytes gives it away -- only the generic kernels need a workspace -- so before
every call it must return 0 for a pinned fused / tiled row and 3*B*C*H*W*4 for a generic one; the unpinned rows run on the
release library, where the Python restatement of choose() says which path is first to fit.

Every row, on NaN-prefilled outputs: all values finite; max |hip - C oracle| <= 4e-6 * 2^level (the bound of
tests/test_gpu_swt.py); at levels <= 3 max |hip - fp64| <= 2 * max |C oracle - fp64| + 1e-7 over the row's batch (the rule of
test_f32_input_and_fp64_accuracy), at levels 4-5 max |hip - fp64| <= 4e-6 * 2^level; the bf16 result is the fp32 result of
the same path rounded, bit for bit; NHWC and NCHW input, and f32 input x / 255 (IEEE, made in NumPy) and u8 input, give the
same bits; the tiled kernel gives the bits of the generic kernels (same taps order, mul then fmaf, axis 0 then axis 1 per
level).  The worst error of every row is printed.
"""
import ctypes

import numpy as np
import pytest
import torch

import swt_fallback_cases as fc
from oracle import swt_np
from wvhash import _lib

pytestmark = pytest.mark.gpu

TORCH_DT = {torch.float32: _lib.WV_DT_F32, torch.bfloat16: _lib.WV_DT_BF16}
OUTS = (torch.float32, torch.bfloat16)
WV_ENOMEM, WV_ENOTSUP = -12, -95


def nan_buffer(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def same_bits(a, b):
    as_int = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return a.dtype == b.dtype and a.shape == b.shape and bool((as_int(a) == as_int(b)).all())


def forward(x, channels_last, wl, lev, out, ws, ws_bytes):
    """wv_swt2d_forward on the current library, exactly these arguments -> return code."""
    lib = _lib.require_gpu()
    B, C, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if channels_last else x.shape
    lo, hi = fc.filters(wl)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, C, 4, H, W)
    return lib.wv_swt2d_forward(_lib.ptr(x), _lib.WV_DT_U8 if x.dtype == torch.uint8 else _lib.WV_DT_F32,
                                _lib.WV_LAYOUT_NHWC if channels_last else _lib.WV_LAYOUT_NCHW, _lib.ptr(out),
                                TORCH_DT[out.dtype], B, C, H, W, lev, _lib.host_floats(lo), _lib.host_floats(hi), len(lo),
                                _lib.ptr(ws), ctypes.c_size_t(ws_bytes), _lib.stream_ptr())


def transform(row, kind, out_dtype, want_ws):
    """The row's batch in the form `kind` through the current library into a NaN buffer; the workspace the library asks for
    must be `want_ws` bytes: the proof of which kernel runs."""
    wl, lev, H, W, C = row
    lib = _lib.require_gpu()
    need = lib.wv_swt2d_workspace_bytes(fc.B, C, H, W, lev, fc.TAPS[wl])
    assert need == want_ws, f"{row} {kind}: workspace of {need} bytes, expected {want_ws}: another kernel than intended runs"
    x, cl = fc.device_input(fc.images(*row), kind)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    out = nan_buffer((fc.B, C, 4, H, W), out_dtype)
    rc = forward(x, cl, wl, lev, out, ws, need)
    assert rc == 0, (row, kind, rc, lib.wv_last_error())
    return out


def check_row(mp, row, pin, path, kinds=fc.KINDS, outs=OUTS):
    """All the checks of the module docstring on one row -> its fp32 result.  `pin`: WV_SWT_PATH (the caller holds the
    diagnostic library) or None (release library); `path`: the kernel the restated planner must name."""
    wl, lev, H, W, C = row
    L = fc.TAPS[wl]
    assert (_lib.require_gpu() is _lib._DIAG) == bool(pin), "a pinned row needs the diag fixture, an unpinned one the release library"
    if pin:
        mp.setenv("WV_SWT_PATH", pin)
    assert {fc.path(L, lev, H, W, C, nhwc, pin) for nhwc in (False, True)} == {path}
    want_ws = fc.workspace_bytes(L, lev, H, W, C, pin)
    assert want_ws == (3 * fc.B * C * H * W * 4 if path == "generic" else 0)
    got = {(kind, od): transform(row, kind, od, want_ws) for kind in kinds for od in outs}
    torch.cuda.synchronize()
    base = got[kinds[0], torch.float32]
    for key, y in got.items():
        assert bool(torch.isfinite(y).all()), f"{row} {key}: values that are not finite (never written?)"
    err = float((base - torch.tensor(fc.reference(*row)).cuda()).abs().max())
    err64 = float(np.abs(base.cpu().numpy().astype(np.float64) - fc.reference64(*row)).max())
    limit64 = 2 * fc.oracle_error(*row) + 1e-7 if lev <= 3 else fc.tol(lev)
    print(f"{path} {wl} L{lev} {H}x{W} B={fc.B} C={C}: max |hip - oracle| = {err:.3e} (bound {fc.tol(lev):.3e}), "
          f"max |hip - fp64| = {err64:.3e} (limit {limit64:.3e})")
    assert err <= fc.tol(lev), f"{row} on {path}: off the C oracle by {err:.3e}"
    assert err64 <= limit64, f"{row} on {path}: off fp64 by {err64:.3e}, limit {limit64:.3e}"
    for (kind, od), y in got.items():
        want = base if od == torch.float32 else base.to(torch.bfloat16)
        assert same_bits(y, want), f"{row} on {path}: {kind} -> {od} differs from {kinds[0]} -> fp32" + \
                                   (" rounded to bf16" if od == torch.bfloat16 else "")
    return base


def generic_result(mp, row):
    """The row's u8 NCHW -> fp32 result from the generic kernels (diagnostic library, WV_SWT_PATH=generic)."""
    wl, lev, H, W, C = row
    with _lib.diagnostic():
        mp.setenv("WV_SWT_PATH", "generic")
        try:
            out = transform(row, "u8_planar", torch.float32, 3 * fc.B * C * H * W * 4)
            torch.cuda.synchronize()
        finally:
            mp.delenv("WV_SWT_PATH")
    return out


def assert_tiled_is_generic(mp, row, tiled):
    assert same_bits(tiled, generic_result(mp, row)), f"{row}: the tiled kernel's bits differ from the generic kernels'"


# ------------------------------------------------------------------------------------------------ tiled
@pytest.mark.parametrize("L,lev", sorted(fc.TILED_CASES))
def test_tiled_every_taps_and_level(L, lev, diag):
    for row in fc.TILED_CASES[(L, lev)]:
        assert_tiled_is_generic(diag, row, check_row(diag, row, "tiled", "tiled"))


@pytest.mark.parametrize("row", fc.TILED_224, ids=lambda r: f"{r[0]}-L{r[1]}")
def test_tiled_level3_big_halo_at_the_workload_size(row, diag):
    assert fc.plan_tiles(fc.TAPS[row[0]], row[1], 224, 224)["lds"] > 64 * 1024
    assert_tiled_is_generic(diag, row, check_row(diag, row, "tiled", "tiled", kinds=("u8_planar",), outs=(torch.float32,)))


@pytest.mark.parametrize("row", fc.TILED_CHANNELS, ids=lambda r: f"{r[0]}-L{r[1]}-C{r[4]}")
def test_tiled_strided_nhwc_channels(row, diag):
    assert_tiled_is_generic(diag, row, check_row(diag, row, "tiled", "tiled"))


@pytest.mark.parametrize("row", fc.TILED_RELEASE, ids=lambda r: f"{r[0]}-L{r[1]}-{r[2]}x{r[3]}")
def test_tiled_is_what_the_release_library_runs(row, monkeypatch):
    assert_tiled_is_generic(monkeypatch, row, check_row(monkeypatch, row, None, "tiled"))


# ------------------------------------------------------------------------------------------------ fused
@pytest.mark.parametrize("L,lev", sorted(fc.FUSED_CASES))
def test_fused_every_config_wide_and_narrow(L, lev, diag):
    for row in fc.FUSED_CASES[(L, lev)]:
        check_row(diag, row, "fused", "fused")


@pytest.mark.parametrize("row", fc.FUSED_CHANNELS, ids=lambda r: f"{r[0]}-L{r[1]}-C{r[4]}")
def test_fused_strided_nhwc_channels(row, diag):
    check_row(diag, row, "fused", "fused")


@pytest.mark.parametrize("L,lev", sorted(fc.FUSED_RELEASE))
def test_fused_is_what_the_release_library_runs_outside_the_window(L, lev, monkeypatch):
    for row in fc.FUSED_RELEASE[(L, lev)]:
        check_row(monkeypatch, row, None, "fused")


# ------------------------------------------------------------------------------------------------ generic
@pytest.mark.parametrize("row,pin", fc.GENERIC_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generic_sizes_taps_levels_channels(row, pin, request):
    if pin:
        check_row(request.getfixturevalue("diag"), row, pin, "generic")
    else:
        check_row(request.getfixturevalue("monkeypatch"), row, None, "generic")


def test_generic_refuses_33_taps_and_writes_nothing():
    wl, lev, H, W, C = fc.REFUSED
    lib = _lib.require_gpu()
    need = lib.wv_swt2d_workspace_bytes(fc.B, C, H, W, lev, 33)
    assert need == 3 * fc.B * C * H * W * 4
    x, cl = fc.device_input(fc.images(*fc.REFUSED), "u8_planar")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for od in OUTS:
        out = nan_buffer((fc.B, C, 4, H, W), od)
        assert forward(x, cl, wl, lev, out, ws, need) == WV_ENOTSUP and b"32 taps" in lib.wv_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and not bool(ws.any())
    ok = nan_buffer((fc.B, C, 4, H, W))                                      # one tap fewer is served
    assert forward(x, cl, "taps32", lev, ok, ws, need) == 0 and bool(torch.isfinite(ok).all())


def test_generic_missing_or_short_workspace_is_enomem_and_writes_nothing():
    row = fc.SHORT_WORKSPACE
    wl, lev, H, W, C = row
    lib = _lib.require_gpu()
    need = lib.wv_swt2d_workspace_bytes(fc.B, C, H, W, lev, fc.TAPS[wl])
    assert need == 3 * fc.B * C * H * W * 4
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for kind in ("u8_planar", "f32_nhwc"):
        x, cl = fc.device_input(fc.images(*row), kind)
        for od in OUTS:
            out = nan_buffer((fc.B, C, 4, H, W), od)
            for w, n in ((None, 0), (None, need), (ws, need - 1), (ws, 0)):
                assert forward(x, cl, wl, lev, out, w, n) == WV_ENOMEM, (kind, od, n)
                assert b"workspace" in lib.wv_last_error()
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and not bool(ws.any())
    assert forward(x, cl, wl, lev, out, ws, need) == 0                        # and with the whole of it: served
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(ws.any())


def test_generic_stride_loop_takes_a_second_turn(diag):
    """B*C*H*W = 1,058,400 elements on a grid capped at 4096 x 256 = 1,048,576 threads: elements from 1,048,576 on, all in the
    last plane, are computed by the second turn of the stride loop of k_planes_to_f32 and k_axis_generic."""
    row = fc.STRIDE_CASE
    wl, lev, H, W, C = row
    diag.setenv("WV_SWT_PATH", "generic")
    got = transform(row, "u8_planar", torch.float32, 3 * fc.B * C * H * W * 4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    planes = fc.sc.unit_planes(fc.images(*row))
    straddling = fc.GRID_CAP // (H * W)
    assert straddling == fc.B * C - 1 and straddling * H * W < fc.GRID_CAP < fc.B * C * H * W
    ref = swt_np.c_transform_planes(planes, fc.filters(wl), lev)              # every plane: first, last = straddling, between
    err = (got.reshape(-1, 4, H, W) - torch.from_numpy(ref).cuda()).abs().flatten(1).amax(dim=1)
    print(f"generic {wl} L{lev} {H}x{W} B={fc.B} C={C}: max |hip - oracle| per plane = "
          + ", ".join(f"{float(e):.3e}" for e in err) + f" (bound {fc.tol(lev):.3e})")
    assert float(err[0]) <= fc.tol(lev) and float(err[straddling]) <= fc.tol(lev) and float(err.max()) <= fc.tol(lev)
    tail = got.reshape(-1, 4, H, W)[straddling].flatten(1)[:, fc.GRID_CAP - straddling * H * W:]     # second turn only
    tail_ref = torch.from_numpy(ref[straddling]).cuda().flatten(1)[:, fc.GRID_CAP - straddling * H * W:]
    assert tail.shape[1] == fc.B * C * H * W - fc.GRID_CAP and float((tail - tail_ref).abs().max()) <= fc.tol(lev)
