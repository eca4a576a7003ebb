"""Shared by tests/test_swt_anchor.py (no GPU) and tests/test_gpu_swt_anchor.py: the one table of identities that ties the
SWT / DWT (oracle/swt_np.py, oracle/swt_oracle.c, the host twins, the HIP kernels) to numbers the REFERENCE itself
produced -- its lifting implementations of haar, Daubechies-4 (= db2) and CDF 9/7 (= bior4.4), run level after level
on LL (tests/golden/lifting_golden.npz, tests/golden/swt_anchor_golden.npz; made by the make_golden_* scripts next to
them).  The decimated transform is the stationary one sampled on the 2^n lattice:

    reference band b of level n at (i, j)
        = f_b * 2^-(n-1) * SWT band b at ((2^n i + o_row) mod H, (2^n j + o_col) mod W)

with (f_LL, f_LH, f_HL, f_HH) = (+1/2, -1, -1, +sqrt 2) -- the reference's 2-D scales (1/2, 1, 1, sqrt 2) times the sign
of its detail filter, which is the opposite of dec_hi for all three wavelets -- the pairing LL <-> cA, LH <-> cH ('da':
axis 0 high), HL <-> cV ('ad'), HH <-> cD, and 2^-(n-1) because each of the n - 1 earlier levels handed on its LL scaled
by 1/2 where the SWT hands on cA as it is.
The offset of an axis depends on the wavelet and on whether the band filters that axis low or high (OFFSET below).

The lifting pads with zeros where the SWT wraps around, so a frame of coefficients along every side of the reference's
arrays differs; FRAME holds its measured width per level and is FIXED: a case that needs a wider frame is a failure to
explain, not a reason to widen it.  Measured with the fp64 oracle on the 224 x 224 cases: residuals off the frame
<= 1.5e-6 at max |x| ~ 4.5 (the reference's own float32 rounding), the next-best alignment off by 0.1 - 7.

DWT (wavedec2, mode 'symmetric'), level 1 only: reference band b at (i, j) = f_b * DWT band b at (i + o_row, j + o_col),
o per axis from DWT_OFFSET, off a border of DWT_FRAME coefficients (symmetric extension there, zero padding here).
At level 2 no alignment exists for db2 / bior4.4: the level-1 approximation is (N + F - 1) // 2 long, which moves the
second decimation to the other phase.

Bounds (both from numbers the suite already uses):
    fp64 oracle against the fixture      2e-6 * max |x|                  (the Haar level-1 anchor of test_oracle_lifting.py)
    float32 implementations add          |f_b| 2^-(n-1) * tol(n) * max(1, max |x|),   tol(n) = 4e-6 * 2^n  (test_gpu_swt.py)
"""
import functools
import os
from collections import namedtuple

import numpy as np

import swt_schedule_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_FILES = {"lifting": "lifting_golden.npz", "anchor": "swt_anchor_golden.npz"}

FACTOR = (0.5, -1.0, -1.0, 2.0 ** 0.5)                 # f_LL, f_LH, f_HL, f_HH
BAND_HIGH = ((False, False), (True, False), (False, True), (True, True))      # band -> (axis 0 high?, axis 1 high?)

# wavelet -> level -> (offset along an axis filtered low, offset along an axis filtered high)
OFFSET = {
    "haar": {1: (0, 0), 2: (0, 0), 3: (0, 0)},
    "bior4.4": {1: (0, 0), 2: (0, 0)},
    "db2": {1: (1, -1), 2: (3, -1), 3: (7, -1)},        # 2^n - 1, -1
}
# wavelet -> level -> coefficients per side the lifting's zero padding corrupts
FRAME = {
    "haar": {1: 0, 2: 0, 3: 0},
    "bior4.4": {1: 2, 2: 3},
    "db2": {1: 1, 2: 2, 3: 2},
}
# DWT level 1: wavelet -> (offset low, offset high), border
DWT_OFFSET = {"haar": (0, 0), "bior4.4": (2, 2), "db2": (1, 0)}
DWT_FRAME = {"haar": 0, "bior4.4": 2, "db2": 1}

Row = namedtuple("Row", "wavelet file case level release_path")
# release_path: the kernel the release library runs for the row's NCHW batch (sliding at 224^2, 64 x 96 and 64 x 48;
# bior4.4 level 2 has no sliding / fused instantiation: tiled; W = 30 is no multiple of 4: generic)
ROWS = [
    Row("haar", "lifting", "haar_224", 1, "slide"), Row("haar", "lifting", "haar_224", 2, "slide"),
    Row("haar", "lifting", "haar_224", 3, "slide"),
    Row("haar", "lifting", "haar_64x48_l2", 1, "slide"), Row("haar", "lifting", "haar_64x48_l2", 2, "slide"),
    Row("bior4.4", "lifting", "cdf97_224", 1, "slide"), Row("bior4.4", "lifting", "cdf97_224", 2, "tiled"),
    Row("bior4.4", "lifting", "cdf97_64x48_l2", 1, "slide"),     # level 2: 16 x 12 arrays leave too little inside the frame
    Row("db2", "anchor", "db2_224", 1, "slide"), Row("db2", "anchor", "db2_224", 2, "slide"),
    Row("db2", "anchor", "db2_224", 3, "slide"),
    Row("db2", "anchor", "db2_64x96", 1, "slide"), Row("db2", "anchor", "db2_64x96", 2, "slide"),
    Row("db2", "anchor", "db2_40x30", 1, "generic"),
]
DWT_ROWS = [r for r in ROWS if r.level == 1]            # every fixture case once, all three wavelets
PINS = ("slide", "fused", "tiled", "generic")


def row_id(r):
    return f"{r.wavelet}-{r.case}-L{r.level}"


@functools.lru_cache(maxsize=None)
def gold(file):
    return np.load(os.path.join(GOLDEN, FIXTURE_FILES[file]))


@functools.lru_cache(maxsize=None)
def case_input(file, case):
    """The case's float32 [N, C, H, W] input, from the seed and shape the fixture stores.  Read-only."""
    import torch
    g = gold(file)
    shape, seed = tuple(int(v) for v in g[f"{case}/shape"]), int(g[f"{case}/seed"])
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).numpy()
    x.setflags(write=False)
    return x


def expected(row):
    """The reference's (LL, LH, HL, HH) of the row's level: float32 [N, C, 4, H / 2^n, W / 2^n]."""
    g = gold(row.file)
    ll, hi = g[f"{row.case}/l{row.level - 1}/ll"], g[f"{row.case}/l{row.level - 1}/hi"]
    return np.concatenate([ll[:, :, None], hi], axis=2)


def swt_to_lattice(y, wavelet, level):
    """SWT result [..., 4, H, W] (cA, cH, cV, cD of `level`) -> what the identity says the reference holds:
    [..., 4, H / 2^n, W / 2^n] float64, each band sampled at its own offsets and scaled by f_b * 2^-(n-1)."""
    y = np.asarray(y, dtype=np.float64)
    H, W = y.shape[-2:]
    step = 1 << level
    off = OFFSET[wavelet][level]
    out = np.empty(y.shape[:-2] + (H // step, W // step), dtype=np.float64)
    for b in range(4):
        rows = (step * np.arange(H // step) + off[BAND_HIGH[b][0]]) % H
        cols = (step * np.arange(W // step) + off[BAND_HIGH[b][1]]) % W
        out[..., b, :, :] = FACTOR[b] * 2.0 ** -(level - 1) * y[..., b, :, :][..., rows[:, None], cols[None, :]]
    return out


def dwt_to_lattice(y, wavelet, h, w):
    """Level-1 DWT result [..., 4, H', W'] -> [..., 4, h, w] float64 on the reference's lattice."""
    y = np.asarray(y, dtype=np.float64)
    off = DWT_OFFSET[wavelet]
    out = np.empty(y.shape[:-2] + (h, w), dtype=np.float64)
    for b in range(4):
        r0, c0 = off[BAND_HIGH[b][0]], off[BAND_HIGH[b][1]]
        assert r0 + h <= y.shape[-2] and c0 + w <= y.shape[-1]
        out[..., b, :, :] = FACTOR[b] * y[..., b, r0:r0 + h, c0:c0 + w]
    return out


def inside(a, frame):
    """[..., h, w] without `frame` coefficients along every side."""
    h, w = a.shape[-2:]
    assert h > 2 * frame and w > 2 * frame
    return a[..., frame:h - frame, frame:w - frame]


def bounds(level, xmax, fp32):
    """Per band: 2e-6 max |x|, plus for a float32 implementation |f_b| 2^-(n-1) tol(n) max(1, max |x|)."""
    base = 2e-6 * xmax
    return [base + (abs(f) * 2.0 ** -(level - 1) * sc.tol(level) * max(1.0, xmax) if fp32 else 0.0) for f in FACTOR]


def residuals(mapped, want, frame):
    """-> max |mapped - want| per band off the frame, over every plane."""
    d = np.abs(inside(mapped, frame) - inside(want.astype(np.float64), frame))
    return [float(d[..., b, :, :].max()) for b in range(4)]


def check(what, row, mapped, frame, fp32):
    """Asserts the identity for one implementation's mapped result, prints the worst residual; -> that residual."""
    x = case_input(row.file, row.case)
    xmax = float(np.abs(x).max())
    want = expected(row)
    assert mapped.shape == want.shape, (what, mapped.shape, want.shape)
    assert np.isfinite(mapped).all(), f"{what} {row_id(row)}: values that are not finite (never written?)"
    res, lim = residuals(mapped, want, frame), bounds(row.level, xmax, fp32)
    print(f"{what} {row_id(row)}: worst residual per band " + ", ".join(f"{r:.3e}" for r in res)
          + " (bounds " + ", ".join(f"{v:.3e}" for v in lim) + f"), max |x| = {xmax:.3f}, frame {frame}")
    for b in range(4):
        assert res[b] <= lim[b], f"{what} {row_id(row)} band {b}: residual {res[b]:.3e} above {lim[b]:.3e}"
    return max(res)


def check_swt(what, row, y, fp32=True):
    return check(what, row, swt_to_lattice(y, row.wavelet, row.level), FRAME[row.wavelet][row.level], fp32)


def check_dwt(what, row, y, fp32=True):
    h, w = expected(row).shape[-2:]
    return check(what, row, dwt_to_lattice(y, row.wavelet, h, w), DWT_FRAME[row.wavelet], fp32)
