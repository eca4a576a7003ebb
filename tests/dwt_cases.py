"""Shared by the DWT tests (CPU and GPU): an independent float64 reference of the decimated DWT and the EDGE case table.

The reference is PyWavelets' documented definition of ``dwt(..., mode='symmetric')`` written with numpy's library
primitives -- ``np.pad(mode='symmetric')``, ``np.convolve``, a strided slice -- and no index arithmetic of its own, so it
shares no formula with the kernel (csrc/dwt.hip), its host twin (csrc/host_twins.cpp) or oracle/swt_np.py, which all
spell out ``(2o + 1 - j) mod 2n`` with a reflection.

Per EDGE case the bound is the rule tests/test_gpu_swt.py uses for the SWT: the library is at least as close to float64
as the float32 mul+add restatement (oracle/swt_np.py), with a factor 2 of slack, plus one float32 ulp of the largest
coefficient for the cases where the restatement happens to be exact:

    |got - ref64|.max() <= 2 * |o32 - ref64|.max() + 2**-23 * |ref64|.max()

All three see the same float32 input planes (uint8 / 255 rounded to float32, float32 as it is) and the same float32
taps, so only accumulation error is measured.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import swt_np
from wvhash.transforms.wavelets import get_filters


# ------------------------------------------------------------------------------------------ float64 reference
def ref_axis(x, f, axis):
    """One decimating pass along `axis` in float64: pad F-1 samples 'symmetric', full convolution, keep every second
    sample from index F on, (n + F - 1) // 2 of them."""
    x, f = np.asarray(x, dtype=np.float64), np.asarray(f, dtype=np.float64)
    n, F = x.shape[axis], f.shape[0]

    def line(v):
        return np.convolve(np.pad(v, F - 1, mode="symmetric"), f)[F::2][:(n + F - 1) // 2]

    return np.apply_along_axis(line, axis, x)


def ref_wavedec2(plane, taps, level):
    """(aa, da, ad, dd) of the last of `level` levels, axis 0 then axis 1 per level, float64 throughout.  `taps` is the
    (dec_lo, dec_hi) pair as the library receives it: rounded to float32, then widened."""
    lo, hi = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in taps)
    a = np.asarray(plane, dtype=np.float64)
    for _ in range(level):
        ta, td = ref_axis(a, lo, 0), ref_axis(a, hi, 0)
        aa, ad = ref_axis(ta, lo, 1), ref_axis(ta, hi, 1)
        da, dd = ref_axis(td, lo, 1), ref_axis(td, hi, 1)
        a = aa
    return aa, da, ad, dd


def out_len(n, F, level):
    for _ in range(level):
        n = (n + F - 1) // 2
    return n


# ------------------------------------------------------------------------------------------------ filter taps
def _seeded_pair(F, seed):
    rng = np.random.default_rng(seed)
    return tuple([float(v) for v in rng.uniform(-1, 1, F).astype(np.float32)] for _ in range(2))


# name -> what dwt2d / dwt2d_host take as `wavelet`: a name the library tabulates or computes, or a (dec_lo, dec_hi) pair
TAPS = {
    "haar": "haar", "db2": "db2", "db4": "db4", "bior4.4": "bior4.4", "db10": "db10",
    "rand32": _seeded_pair(32, 101), "rand3": _seeded_pair(3, 103), "rand5": _seeded_pair(5, 105),
}


def taps32(name):
    """(dec_lo, dec_hi) float32 arrays: the taps as the library receives them."""
    lo, hi = get_filters(TAPS[name])
    return np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)


def flen(name):
    return len(taps32(name)[0])


# --------------------------------------------------------------------------------------------------- EDGE table
Case = namedtuple("Case", "idx taps H W level channels_last C B dtype")


def case_id(c):
    return (f"{c.taps}-{c.H}x{c.W}-l{c.level}-{'nhwc' if c.channels_last else 'nchw'}-c{c.C}-b{c.B}-"
            f"{'u8' if c.dtype == np.uint8 else 'f32'}")


def _edge_table():
    rows = []                                                   # (taps, H, W, level)
    big = [(1, 64), (64, 1), (37, 51), (50, 38)]
    for t, name in enumerate(TAPS):
        F = flen(name)
        # the sizes at which some axis is shorter than the filter, so that the reflection repeats: with every filter
        short = [(1, 1), (1, 2), (2, 1), (3, 5), (F - 1, F - 1), (F, F + 1)]
        for hw in dict.fromkeys(short):
            rows.append((name, *hw, 1))
        for k in range(2):                                      # the four larger sizes: twice each over the eight filters
            rows.append((name, *big[(2 * t + k) % 4], 1))
    # one level past the fixed point of n -> (n + F - 1) // 2 (F - 2 from below), from a size below it
    rows += [("db4", 5, 3, 6), ("db2", 1, 1, 3), ("bior4.4", 3, 5, 5)]
    # the deepest level the ABI takes
    rows += [("db4", 1, 2, 12), ("haar", 5, 3, 12)]
    # layout x channels x batch x dtype: all 32 combinations in turn, so each layout / dtype pair comes up many times
    combos = [(cl, C, B, dt) for dt in (np.uint8, np.float32) for B in (1, 3) for C in (1, 2, 3, 4) for cl in (False, True)]
    step = 11                                                   # odd: walks all 32 before it repeats
    return [Case(i, *row, *combos[(i * step) % len(combos)]) for i, row in enumerate(rows)]


EDGE = _edge_table()
EDGE_IDS = [case_id(c) for c in EDGE]

for _c in EDGE:                                                 # the table keeps what its comments promise
    if _c.level > 1 and _c.level < 12:
        _F = flen(_c.taps)
        assert (out_len(_c.H, _F, _c.level - 2), out_len(_c.W, _F, _c.level - 2)) == (_F - 2, _F - 2), _c
        assert _c.H < _F - 2 and _c.W < _F - 2, _c
assert {(c.channels_last, c.C, c.B, c.dtype) for c in EDGE} == {(cl, C, B, dt) for cl in (False, True) for C in (1, 2, 3, 4)
                                                                for B in (1, 3) for dt in (np.uint8, np.float32)}


def case_input(c):
    """The case's input in its own layout: uint8 0..255, or float32 in (-1e3, 1e3) used as it is.  Read-only."""
    rng = np.random.default_rng(1000 + c.idx)
    shape = (c.B, c.H, c.W, c.C) if c.channels_last else (c.B, c.C, c.H, c.W)
    if c.dtype == np.uint8:
        x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    else:
        x = rng.uniform(-1e3, 1e3, size=shape).astype(np.float32)
    x.flags.writeable = False
    return x


def planes_f32(c, x):
    """[B, C, H, W] float32: the planes the transform starts from (uint8 / 255 in float32)."""
    p = np.ascontiguousarray(x.transpose(0, 3, 1, 2)) if c.channels_last else x
    return p.astype(np.float32) / np.float32(255) if c.dtype == np.uint8 else p


@functools.lru_cache(maxsize=None)
def references(idx):
    """-> (x, ref64 [B,C,4,h,w] float64, o32 [B,C,4,h,w] float32) of EDGE[idx], computed once, read-only."""
    c = EDGE[idx]
    x = case_input(c)
    p = planes_f32(c, x)
    taps = taps32(c.taps)
    ref = np.stack([np.stack([np.stack(ref_wavedec2(p[b, ch], taps, c.level)) for ch in range(c.C)]) for b in range(c.B)])
    o32 = np.stack([np.stack([swt_np.wavedec2_coarsest(p[b, ch], taps, c.level, np.float32) for ch in range(c.C)])
                    for b in range(c.B)])
    ref.flags.writeable = False
    o32.flags.writeable = False
    return x, ref, o32


def error_and_bound(got, ref64, o32):
    """-> (|got - ref64|.max(), the bound of the module docstring)."""
    ref_max = float(np.abs(ref64).max())
    bound = 2 * float(np.abs(o32.astype(np.float64) - ref64).max()) + 2.0 ** -23 * ref_max
    return float(np.abs(got.astype(np.float64) - ref64).max()), bound


def bits(a):
    """int32 view of a float32 array or tensor on the host."""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)
