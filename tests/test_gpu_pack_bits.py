"""wv_pack_bits and wv_bit_counts (csrc/hamming.hip: k_pack_bits, k_bit_counts) called directly through ctypes against numpy:
row-strided sources, more (row, word) items than a launch has waves, more rows than one pass of the counting grid covers,
pad bits, the bad_flag rule, and outputs pre-filled in front of a sentinel tail.  The host twins get the same inputs."""
import numpy as np
import pytest
import torch

from wvhash import _lib

pytestmark = pytest.mark.gpu

TAIL = 1024                                                       # sentinel elements behind every output (>= 4 KB)
FILL64, TAIL64 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64(0x0123456789ABCDEF)
FILL32, TAIL32 = np.uint32(0x5A5A5A5A), np.uint32(0x0BADF00D)
EXTRA = 5                                                         # columns of the strided source beyond nbits


def np_pack(v, nbits):
    """numpy's little-endian packing of v[:, :nbits] > 0 -> uint64 [rows, words]; pad bits 0."""
    words = (nbits + 63) // 64
    bits = np.zeros((v.shape[0], words * 64), np.uint8)
    with np.errstate(invalid="ignore"):
        bits[:, :nbits] = v[:, :nbits] > 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(v.shape[0], words)


def source(rows, nbits, mode, strided, seed):
    """Clean values (+-1 codes / 0-1 labels).  strided: the first nbits columns of a matrix EXTRA columns wider, whose other
    columns hold what must never be read: positive values (they would show up as pad bits) and values bad_flag objects to."""
    g = np.random.default_rng(seed)
    v = g.integers(0, 2, (rows, nbits + (EXTRA if strided else 0))).astype(np.float32)
    if mode == 0:
        v = 2 * v - 1
    if strided:
        v[:, nbits:] = [0.5, np.nan, 0.0, 0.5, 0.5] if mode == 0 else [-1.0, 3.0, -2.0, 3.0, -1.0]
    return v


def pack(v, nbits, mode, where):
    """-> (uint64 [rows, words], flag) from wv_pack_bits ("gpu") or wv_pack_bits_cpu; checks the sentinel tails."""
    lib = _lib.load()
    rows, ld = v.shape
    words = (nbits + 63) // 64
    out = np.concatenate([np.full(rows * words, FILL64), np.full(TAIL, TAIL64)])
    flag = np.concatenate([np.zeros(1, np.int32), np.full(TAIL, TAIL32).view(np.int32)])
    if where == "gpu":
        d_v, d_out, d_flag = (torch.from_numpy(a).cuda() for a in (v, out.view(np.int64), flag))
        rc = lib.wv_pack_bits(_lib.ptr(d_v), ld, _lib.ptr(d_out), rows, nbits, mode, _lib.ptr(d_flag), _lib.stream_ptr())
        torch.cuda.synchronize()
        out, flag = d_out.cpu().numpy().view(np.uint64), d_flag.cpu().numpy()
    else:
        rc = lib.wv_pack_bits_cpu(v.ctypes.data, ld, out.ctypes.data, rows, nbits, mode, flag.ctypes.data)
    assert rc == 0, rc
    assert np.all(out[rows * words:] == TAIL64) and np.all(flag[1:].view(np.uint32) == TAIL32), "written past the end"
    return out[:rows * words].reshape(rows, words), int(flag[0])


@pytest.mark.parametrize("nbits", [1, 63, 64, 65, 96, 250])
@pytest.mark.parametrize("rows", [1, 3, 3000])
def test_pack_bits_against_numpy(rows, nbits):
    """3000 rows of 250 bits are 12,000 (row, word) items for the 8192 waves of a launch: the wave-stride loop."""
    for mode in (0, 1):
        for strided in (False, True):
            v = source(rows, nbits, mode, strided, seed=rows + 7 * nbits + mode)
            assert v.strides[0] == 4 * (nbits + EXTRA * strided)
            want = np_pack(v, nbits)
            for where in ("gpu", "cpu"):
                got, flag = pack(v, nbits, mode, where)
                assert np.array_equal(got, want), (mode, strided, where)
                assert flag == 0, (mode, strided, where)              # clean inside nbits, whatever the extra columns hold
            if nbits % 64:
                assert not np.any(want[:, -1] >> np.uint64(nbits % 64))


@pytest.mark.parametrize("rows,nbits,at", [(3, 65, (2, 64)), (3, 65, (0, 0)), (3000, 250, (2999, 249)), (3000, 250, (2100, 3))])
def test_pack_bits_bad_flag(rows, nbits, at):
    """Mode 0 (codes) objects to anything but +-1 -- a 0, a NaN, a 0.5 -- and mode 1 (labels) to a negative value, inside nbits
    only; the words are still the packing of v > 0."""
    for mode, bad_values in ((0, (0.0, np.nan, 0.5)), (1, (-1.0,))):
        for bad in bad_values:
            v = source(rows, nbits, mode, True, seed=11)
            v[at] = bad
            for where in ("gpu", "cpu"):
                got, flag = pack(v, nbits, mode, where)
                assert flag == 1, (mode, bad, where)
                assert np.array_equal(got, np_pack(v, nbits)), (mode, bad, where)


def counts_of(packed, nbits, where):
    lib = _lib.load()
    rows = packed.shape[0]
    counts = np.concatenate([np.full(nbits, FILL32), np.full(TAIL, TAIL32)])
    if where == "gpu":
        d_p, d_c = torch.from_numpy(packed.view(np.int64)).cuda(), torch.from_numpy(counts.view(np.int32)).cuda()
        rc = lib.wv_bit_counts(_lib.ptr(d_p), rows, nbits, _lib.ptr(d_c), _lib.stream_ptr())
        torch.cuda.synchronize()
        counts = d_c.cpu().numpy().view(np.uint32)
    else:
        rc = lib.wv_bit_counts_cpu(packed.ctypes.data, rows, nbits, counts.ctypes.data)
    assert rc == 0, rc
    assert np.all(counts[nbits:] == TAIL32), "counts beyond nbits touched"
    return counts[:nbits]


@pytest.mark.parametrize("nbits", [16, 64, 96, 250])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 70001])
def test_bit_counts_against_column_sums(rows, nbits):
    """Random 64-bit words, so the pad bits of the last word are set and must not be counted; counts pre-filled with a non-zero
    pattern; 70,001 rows are more than the 65,536 one pass of the grid covers."""
    words = (nbits + 63) // 64
    packed = np.random.default_rng(rows + nbits).integers(0, 2 ** 64, (rows, words), dtype=np.uint64)
    if nbits % 64:
        assert np.any(packed[:, -1] >> np.uint64(nbits % 64))
    bits = np.unpackbits(packed.view(np.uint8).reshape(rows, words * 8), axis=1, bitorder="little")[:, :nbits]
    want = bits.sum(axis=0, dtype=np.int64)
    for where in ("gpu", "cpu"):
        assert np.array_equal(counts_of(packed, nbits, where).astype(np.int64), want), where
