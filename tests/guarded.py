"""Guarded buffers for the buffer-contract tests (test_buffer_contract_host.py, test_gpu_buffer_contract.py).
No test functions, no fixtures: a plain helper.

A placed buffer is one uint8 allocation [guard | payload | guard]: the guards are GUARD bytes (64 KiB) of 0xA5 on either
side, the payload starts at a 256-byte boundary plus `offset` -- so `offset` alone decides its alignment -- and is pre-filled
with a byte pattern (0x00 / 0xFF: 0xFF reads as NaN in floats, -1 in ints, 65535 in uint16 rows).  A pitched buffer has its
row gaps (columns cols..ld of every row) filled and checked like guards.  assert_intact() compares every guard and gap byte
of every buffer placed through the registry and names the buffer and the first changed offset (relative to the payload's
first byte: negative = in front of it).  Works the same on host and on device tensors.
"""
import torch

GUARD = 64 * 1024
ALIGN = 256
GUARD_BYTE = 0xA5


class GuardError(AssertionError):
    pass


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class _Placed:
    def __init__(self, name, raw, start, nbytes, row_bytes=None, pitch_bytes=None, rows=0):
        self.name, self.raw, self.start, self.nbytes = name, raw, start, nbytes
        self.row_bytes, self.pitch_bytes, self.rows = row_bytes, pitch_bytes, rows

    def first_damage(self):
        """-> None, or (where, offset relative to the payload's first byte) of the first changed guard / gap byte"""
        raw, lo, hi = self.raw, self.start, self.start + self.nbytes
        front = (raw[:lo] != GUARD_BYTE).nonzero()
        if front.numel():
            return "front guard", int(front[0]) - lo
        if self.pitch_bytes and self.rows > 1 and self.pitch_bytes > self.row_bytes:
            body = raw[lo:lo + (self.rows - 1) * self.pitch_bytes].view(self.rows - 1, self.pitch_bytes)
            gap = (body[:, self.row_bytes:] != GUARD_BYTE).nonzero()
            if gap.numel():
                r, c = int(gap[0, 0]), int(gap[0, 1])
                return f"pitch gap of row {r}", r * self.pitch_bytes + self.row_bytes + c
        back = (raw[hi:] != GUARD_BYTE).nonzero()
        if back.numel():
            return "back guard", self.nbytes + int(back[0])
        return None


class Guards:
    """The registry of one test: every buffer placed through it is checked by assert_intact()."""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.placed = []

    def _raw(self, nbytes, offset, dtype, device):
        assert offset >= 0 and offset % _itemsize(dtype) == 0, "offset: a whole number of elements"
        device = self.device if device is None else torch.device(device)
        raw = torch.full((GUARD + ALIGN + offset + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
        start = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN + offset
        raw = raw[:start + nbytes + GUARD]                     # the back guard is exactly GUARD bytes
        return raw, start

    def place(self, nbytes_or_shape, dtype=torch.uint8, device=None, offset=0, fill=0x00, name=None):
        """-> a contiguous tensor of `dtype` whose data_ptr() is (a 256-byte boundary) + offset, every byte = fill.
        nbytes_or_shape: an int (elements of dtype; bytes for uint8) or a shape."""
        shape = (int(nbytes_or_shape),) if isinstance(nbytes_or_shape, int) else tuple(int(s) for s in nbytes_or_shape)
        nbytes = _numel(shape) * _itemsize(dtype)
        raw, start = self._raw(nbytes, offset, dtype, device)
        raw[start:start + nbytes] = fill
        view = raw[start:start + nbytes].view(dtype).view(shape)
        assert view.data_ptr() % ALIGN == offset % ALIGN
        self.placed.append(_Placed(name or f"buffer{len(self.placed)}", raw, start, nbytes))
        return view

    def place_like(self, t, device=None, offset=0, name=None):
        """a placed copy of the (contiguous) tensor t"""
        v = self.place(tuple(t.shape), t.dtype, device, offset, 0x00, name)
        v.copy_(t)
        return v

    def pitched(self, rows, cols, ld, dtype, device=None, offset=0, fill=0x00, name=None):
        """-> a [rows, cols] view with row pitch ld (elements) of one placed buffer of (rows - 1) * ld + cols elements; the
        gap elements cols..ld of every row but the last hold guard bytes and are checked by assert_intact()."""
        assert ld >= cols and rows >= 1
        isz = _itemsize(dtype)
        n = (rows - 1) * ld + cols
        raw, start = self._raw(n * isz, offset, dtype, device)
        flat = raw[start:start + n * isz].view(dtype)
        view = torch.as_strided(flat, (rows, cols), (ld, 1))
        view.copy_(torch.full((rows, cols * isz), fill, dtype=torch.uint8, device=raw.device).view(dtype))
        self.placed.append(_Placed(name or f"buffer{len(self.placed)}", raw, start, n * isz, cols * isz, ld * isz, rows))
        return view

    def assert_intact(self):
        for p in self.placed:
            hit = p.first_damage()
            if hit is not None:
                raise GuardError(f"{p.name}: {hit[0]} changed at byte offset {hit[1]} of the payload "
                                 f"(payload {p.nbytes} bytes at {p.raw.data_ptr() + p.start:#x})")


def bits(t):
    """the tensor's bytes, for bit-for-bit comparisons of any dtype (contiguous or a pitched view)"""
    return t.contiguous().view(torch.uint8)
