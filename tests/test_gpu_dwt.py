"""GPU: wv_dwt2d_forward (DWTTransform) against the numpy restatement of pywt.wavedec2's coarsest level; and, over the EDGE
table of tests/dwt_cases.py, against its host twin (the same bits; as found, they agreed on every case) and an independent
float64 reference, with the grid-stride branch, guarded buffers, the plugin and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import dwt_cases as D
from oracle import swt_np

pytestmark = pytest.mark.gpu

TOL = 2e-6   # fp32 taps, fma vs mul+add accumulation, at most 3 levels * 2 axes * 10 taps


@pytest.mark.parametrize("wavelet,level,shape", [
    ("haar", 1, (2, 3, 32, 32)), ("haar", 2, (1, 3, 224, 224)), ("db2", 1, (2, 3, 40, 56)),
    ("db2", 3, (1, 3, 224, 224)), ("db4", 2, (1, 2, 37, 51)), ("bior4.4", 1, (1, 1, 64, 48)),
    ("db4", 1, (1, 1, 3, 5)),
])
def test_dwt_matches_oracle(wavelet, level, shape):
    from wvhash.transforms import dwt2d
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    got = dwt2d(torch.from_numpy(x).cuda(), wavelet, level).cpu().numpy()
    for b in range(shape[0]):
        for c in range(shape[1]):
            exp = swt_np.wavedec2_coarsest(x[b, c].astype(np.float32) / np.float32(255), wavelet, level)
            assert got[b, c].shape == exp.shape
            np.testing.assert_allclose(got[b, c], exp, atol=TOL * 2 ** level, rtol=0)


def test_dwt_layouts_and_float_input():
    from wvhash.transforms import dwt2d
    rng = np.random.default_rng(4)
    x = rng.random((2, 3, 48, 64), dtype=np.float32)
    a = dwt2d(torch.from_numpy(x).cuda(), "db2", 2)
    b = dwt2d(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda(), "db2", 2, channels_last=True)
    assert torch.equal(a, b)
    exp = swt_np.wavedec2_coarsest(x[1, 2], "db2", 2)
    np.testing.assert_allclose(a[1, 2].cpu().numpy(), exp, atol=8e-6, rtol=0)


def test_dwt_transform_class_and_errors():
    from wvhash import _lib
    from wvhash.transforms import DWTTransform
    img = np.random.default_rng(5).integers(0, 256, size=(30, 45, 3), dtype=np.uint8)   # fix_size -> 32 x 48
    t = DWTTransform(level=2, wavelet="haar", device="cuda")
    from PIL import Image
    out = t(Image.fromarray(img))
    assert out.shape == (3, 4, 8, 12) and out.dtype == torch.float32
    lib = _lib.require_gpu()
    x = torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device="cuda")
    o = torch.empty((1, 1, 4, 4, 4), device="cuda")
    f = _lib.host_floats([0.5, 0.5])
    assert lib.wv_dwt2d_forward(_lib.ptr(x), 0, 0, _lib.ptr(o), 1, 1, 8, 8, 1, f, f, 2, None, 0, None) == -12
    assert lib.wv_dwt2d_forward(_lib.ptr(x), 0, 0, _lib.ptr(o), 1, 1, 8, 8, 0, f, f, 2, None, 0, None) == -22


# ------------------------------------------------------------------------------------------------------------------
# The kernel against its host twin (the same bits) and against the independent float64 reference of tests/dwt_cases.py
def _on_gpu(case, x):
    from wvhash.transforms import dwt2d
    return dwt2d(torch.from_numpy(x.copy()).cuda(), D.TAPS[case.taps], case.level, channels_last=case.channels_last)


def _on_host(case, x):
    from wvhash.transforms import dwt2d_host
    return dwt2d_host(torch.from_numpy(x.copy()), D.TAPS[case.taps], case.level, channels_last=case.channels_last)


@pytest.mark.parametrize("case", D.EDGE, ids=D.EDGE_IDS)
def test_kernel_and_twin_give_the_same_bits(case):
    """Every EDGE case through dwt2d and dwt2d_host: what a DataLoader worker (twin) and the main process (kernel) hand a
    model must not differ in one bit.  The kernel is also held to the twin's bound against float64."""
    x, ref64, o32 = D.references(case.idx)
    got, host = _on_gpu(case, x), _on_host(case, x)
    assert got.shape == host.shape == ref64.shape
    diff = D.bits(got) != D.bits(host)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[0])
    err, bound = D.error_and_bound(got.cpu().numpy(), ref64, o32)
    print(f"{D.case_id(case)}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)


def test_grid_stride_loops_serve_what_the_capped_grid_leaves():
    """3.1M inputs and 1.6M first-pass outputs against the 4096 x 256 = 1,048,576 threads dwt_grid caps a launch at: the
    conversion goes round its stride loop three times, the first axis pass twice.  Every plane against the twin; the last
    plane, which no thread reaches on its first round, against float64 as well."""
    from wvhash.transforms import dwt2d, dwt2d_host
    B, C, H, W, level = 4, 3, 512, 512, 2
    assert B * C * H * W > 4096 * 256 and B * C * D.out_len(H, 4, 1) * W > 4096 * 256
    x = np.random.default_rng(77).integers(0, 256, size=(B, H, W, C), dtype=np.uint8)
    got = dwt2d(torch.from_numpy(x).cuda(), "db2", level, channels_last=True)
    host = dwt2d_host(torch.from_numpy(x), "db2", level, channels_last=True)
    assert tuple(got.shape) == (B, C, 4, D.out_len(H, 4, level), D.out_len(W, 4, level))
    diff = D.bits(got) != D.bits(host)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[0])
    plane = x[3, :, :, 2].astype(np.float32) / np.float32(255)
    taps = D.taps32("db2")
    ref64 = np.stack(D.ref_wavedec2(plane, taps, level))
    o32 = swt_np.wavedec2_coarsest(plane, taps, level, np.float32)
    err, bound = D.error_and_bound(got[3, 2].cpu().numpy(), ref64, o32)
    print(f"grid stride, plane (3, 2): err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)


GUARD = 1 << 20


def test_dwt_keeps_to_the_workspace_and_output_sizes_it_reports():
    """wv_dwt2d_forward through ctypes on a ragged case (37 x 51, db4, two levels: no size is a multiple of anything), with
    workspace_bytes exactly as wv_dwt2d_workspace_bytes reports and the output at the front of a larger buffer; 1 MiB of
    0xA5 follows each.  The wrapper's bits, not one guard byte changed, the input untouched."""
    from wvhash import _lib
    from wvhash.transforms import dwt2d
    lib = _lib.require_gpu()
    B, C, H, W, level = 2, 3, 37, 51, 2
    lo, hi = D.taps32("db4")
    x = torch.from_numpy(np.random.default_rng(78).integers(0, 256, size=(B, C, H, W), dtype=np.uint8)).cuda()
    x0 = x.clone()
    want = dwt2d(x, "db4", level)
    n_out = want.numel() * 4
    need = lib.wv_dwt2d_workspace_bytes(B, C, H, W, level, len(lo))
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((n_out + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.wv_dwt2d_forward(_lib.ptr(x), _lib.WV_DT_U8, _lib.WV_LAYOUT_NCHW, _lib.ptr(out), B, C, H, W, level,
                              _lib.host_floats(lo), _lib.host_floats(hi), len(lo), _lib.ptr(ws), ctypes.c_size_t(need),
                              _lib.stream_ptr())
    assert rc == 0, lib.wv_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32))
    assert bool((out[n_out:] == 0xA5).all()) and bool((ws[need:] == 0xA5).all())
    assert torch.equal(x, x0)


def test_plugin_gives_the_same_bits_on_the_gpu_and_on_the_host():
    from PIL import Image
    from wvhash.transforms import DWTTransform
    img = Image.fromarray(np.random.default_rng(79).integers(0, 256, size=(30, 45, 3), dtype=np.uint8))   # fix_size -> 32 x 48
    on_gpu = DWTTransform(level=2, wavelet="db2", device="cuda")(img)
    on_host = DWTTransform(level=2, wavelet="db2", device="cpu")(img)
    assert not on_gpu.is_cuda and not on_host.is_cuda
    assert tuple(on_gpu.shape) == tuple(on_host.shape) == (3, 4, D.out_len(32, 4, 2), D.out_len(48, 4, 2))
    assert np.array_equal(D.bits(on_gpu), D.bits(on_host))


def test_device_entry_refuses_bad_arguments_before_any_launch():
    """Each refused call leaves the sentinel in `out` and in the workspace: nothing was launched."""
    from wvhash import _lib
    lib = _lib.require_gpu()
    x = torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device="cuda")
    need = lib.wv_dwt2d_workspace_bytes(1, 1, 8, 8, 12, 32)            # enough for every call below, were it accepted
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    o = torch.full((4 * 31 * 31,), -3.0, device="cuda")
    f = _lib.host_floats([0.5] * 33)

    def call(dtype=_lib.WV_DT_U8, layout=_lib.WV_LAYOUT_NCHW, level=1, taps=2, ws_bytes=need):
        return lib.wv_dwt2d_forward(_lib.ptr(x), dtype, layout, _lib.ptr(o), 1, 1, 8, 8, level, f, f, taps, _lib.ptr(ws),
                                    ctypes.c_size_t(ws_bytes), _lib.stream_ptr())

    assert call(level=13) == -22
    assert call(taps=1) == -22 and call(taps=33) == -22
    assert call(dtype=2) == -22
    assert call(layout=7) == -22 and call(layout=-1) == -22 and call(layout=2) == -22
    assert call(ws_bytes=lib.wv_dwt2d_workspace_bytes(1, 1, 8, 8, 1, 2) - 1) == -12
    torch.cuda.synchronize()
    assert bool((o == -3.0).all()) and bool((ws == 0xA5).all())
    assert call(layout=_lib.WV_LAYOUT_NHWC) == 0                        # the same call with arguments in range goes through
    torch.cuda.synchronize()
    assert bool((o[:4 * 4 * 4] != -3.0).all()) and bool((o[4 * 4 * 4:] == -3.0).all())
