"""GPU: wv_rawstack_forward (RawStackTransform) against its host twin wv_rawstack_forward_cpu, bit for bit: 1, 3 and 4
channels, both layouts, uint8 (divided by 255 on the device and on the host) and float32, a launch larger than the grid cap,
a guarded output, and the layout check."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1 << 20


def _input(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return torch.from_numpy(rng.integers(0, 256, size=shape, dtype=np.uint8))
    return torch.from_numpy(rng.uniform(-1e3, 1e3, size=shape).astype(np.float32))     # used as it is, not rescaled


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("copies", [1, 5])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_rawstack_equals_its_twin(C, channels_last, dtype, copies):
    from wvhash.transforms import rawstack, rawstack_host
    B, H, W = 2, 6, 10
    x = _input((B, H, W, C) if channels_last else (B, C, H, W), dtype, 10 * C + copies)
    got = rawstack(x.cuda(), copies, channels_last=channels_last)
    host = rawstack_host(x, copies, channels_last=channels_last)
    assert tuple(got.shape) == (B, C, copies, H, W) and _same_bits(got, host)
    planes = x.numpy().transpose(0, 3, 1, 2) if channels_last else x.numpy()   # ... and the twin is the plain definition
    planes = planes.astype(np.float32) / np.float32(255) if dtype == np.uint8 else planes
    want = np.broadcast_to(planes[:, :, None], (B, C, copies, H, W)).copy()
    assert _same_bits(host, torch.from_numpy(want))


def test_rawstack_above_the_grid_cap():
    """1,572,864 pixels against the 4096 x 256 = 1,048,576 threads a launch is capped at: the stride loop's second round."""
    from wvhash.transforms import rawstack, rawstack_host
    B, C, H, W, copies = 2, 3, 512, 512, 2
    assert B * C * H * W > 4096 * 256
    x = _input((B, H, W, C), np.uint8, 5)
    assert _same_bits(rawstack(x.cuda(), copies, channels_last=True), rawstack_host(x, copies, channels_last=True))


def test_rawstack_writes_its_output_and_nothing_behind_it():
    from wvhash import _lib
    from wvhash.transforms import rawstack
    lib = _lib.require_gpu()
    B, C, H, W, copies = 2, 3, 37, 51, 5
    x = _input((B, H, W, C), np.uint8, 6).cuda()
    x0 = x.clone()
    want = rawstack(x, copies, channels_last=True)
    n_out = want.numel() * 4
    out = torch.full((n_out + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.wv_rawstack_forward(_lib.ptr(x), _lib.WV_DT_U8, _lib.WV_LAYOUT_NHWC, _lib.ptr(out), _lib.WV_DT_F32, B, C, H, W,
                                 copies, _lib.stream_ptr())
    assert rc == 0, lib.wv_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32))
    assert bool((out[n_out:] == 0xA5).all()) and torch.equal(x, x0)


def test_rawstack_refuses_an_unknown_layout_before_any_launch():
    from wvhash import _lib
    lib = _lib.require_gpu()
    x = torch.zeros((1, 3, 6, 10), dtype=torch.uint8, device="cuda")
    o = torch.full((1, 3, 2, 6, 10), -3.0, device="cuda")

    def call(layout):
        return lib.wv_rawstack_forward(_lib.ptr(x), _lib.WV_DT_U8, layout, _lib.ptr(o), _lib.WV_DT_F32, 1, 3, 6, 10, 2,
                                       _lib.stream_ptr())

    assert call(7) == -22 and call(-1) == -22 and call(2) == -22
    torch.cuda.synchronize()
    assert bool((o == -3.0).all())
    assert call(_lib.WV_LAYOUT_NHWC) == 0
    torch.cuda.synchronize()
    assert bool((o == 0.0).all())
