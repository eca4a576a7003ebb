"""Shared by tests/test_swt_fallback_cases.py (no GPU) and tests/test_gpu_swt_fallback.py: the planner of csrc/swt.hip and
csrc/swt_fused.hip restated in plain Python (swt_config, fused_fits, pick_shape, tile_lds_bytes, plan_tiles, choose; the
sliding window comes from swt_schedule_cases.fits), the case tables that drive the three fallback SWT implementations
(register-fused, tiled, generic) to their tile edges, seeded inputs in the four input forms, and two references: the C
oracle plane by plane and the fp64 NumPy restatement.

A table row is (wavelet, level, H, W, C); B = 2 throughout.  What each row is there for is asserted, without a GPU, by
tests/test_swt_fallback_cases.py.
"""
import functools

import numpy as np

import swt_schedule_cases as sc

B = 2
TAPS = dict(sc.TAPS)
NAME_OF_TAPS = {n: wl for wl, n in sc.TAPS.items()}
tol = sc.tol
KINDS = ("u8_planar", "u8_nhwc", "f32_planar", "f32_nhwc")      # {u8, f32} x {NCHW, NHWC}; all of them for any C here

# ------------------------------------------------------------------------------------------------ the planner, restated
CONFIGS = [(4, 3), (2, 1), (4, 1), (4, 2), (2, 2), (2, 3), (8, 1), (10, 1)]          # WV_SWT_CONFIGS (csrc/swt.hpp)
TILED_TAPS, TILED_LEVELS = (2, 4, 8, 10), (1, 2, 3)                                  # dispatch_taps / dispatch_levels
FUSED_TH, FUSED_WIDE, FUSED_NARROW = 32, 112, 64
MAX_LDS = 160 * 1024                                                                 # kMaxLdsBytes
TWO_PER_CU = 78 * 1024
GRID_CAP = 4096 * 256                                                                # grid_for: threads of one generic launch


def swt_config(L, level):
    return (L, level) in CONFIGS


def fused_fits(L, level, W):
    return swt_config(L, level) and W % 4 == 0


def fused_plan(H, W):
    """pick_shape + launch_fused -> dict(kind, TW, tilesX, tilesY, last_w, last_h): the tile and how much of the last one
    lies inside the image."""
    waste112 = -(-W // FUSED_WIDE) * FUSED_WIDE - W
    waste64 = -(-W // FUSED_NARROW) * FUSED_NARROW - W
    wide = waste112 * FUSED_NARROW <= waste64 * FUSED_WIDE
    TW = FUSED_WIDE if wide else FUSED_NARROW
    tx, ty = -(-W // TW), -(-H // FUSED_TH)
    return dict(kind="wide" if wide else "narrow", TW=TW, tilesX=tx, tilesY=ty, last_w=W - (tx - 1) * TW,
                last_h=H - (ty - 1) * FUSED_TH)


def _up4(v):
    return (v + 3) // 4 * 4


def tile_lds_bytes(L, level, TH, TW):
    """-> (dynamic LDS bytes of k_swt_tiled, RH, RW)."""
    span = (1 << level) - 1
    HB, HA = (L // 2 - 1) * span, (L // 2) * span
    CB = _up4(HB)
    RW = _up4(CB + TW + HA)
    RH = HB + TH + HA
    G = _up4((1 << (level - 1)) * (L // 2) + 8)
    return (2 * (RH * RW + 2 * G) + TH * RW + 2 * G) * 4, RH, RW


def plan_tiles(L, level, H, W):
    """plan_tiles of csrc/swt.hip -> None (the tiled kernel does not take the shape) or dict(TH, TW, tilesX, tilesY, lds,
    last_w, last_h, halo_rows)."""
    if L not in TILED_TAPS or level not in TILED_LEVELS or W % 4:
        return None
    lds = lambda th, tw: tile_lds_bytes(L, level, th, tw)[0]
    tilesX = -(-W // 128)
    TW = _up4(-(-W // tilesX))
    TH = min(H, 32)
    while TH > 8 and lds(TH, TW) > TWO_PER_CU:
        TH -= 8
    if lds(TH, TW) > TWO_PER_CU:
        TH = min(H, 32)
        while TH > 4 and lds(TH, TW) > MAX_LDS - 1024:
            TH -= 4
    TW = min(TW, W)
    tilesX = -(-W // TW)
    nbytes, RH, RW = tile_lds_bytes(L, level, TH, TW)
    if nbytes > MAX_LDS - 1024 or RH * (RW // 4) * 4 >= (1 << 32) // (RW // 4 + 1):
        return None
    tilesY = -(-H // TH)
    return dict(TH=TH, TW=TW, tilesX=tilesX, tilesY=tilesY, lds=nbytes, last_w=W - (tilesX - 1) * TW,
                last_h=H - (tilesY - 1) * TH, halo_rows=RH - TH)


def slide_fits(L, level, H, W, C=3, nhwc=False):
    return swt_config(L, level) and (not nhwc or C == 3) and sc.fits(NAME_OF_TAPS[L], level, H, W)


def path(L, level, H, W, C=3, nhwc=False, pin=None):
    """choose() of csrc/swt.hip: the first of slide, fused, tiled that fits, else generic; with `pin` (WV_SWT_PATH of the
    diagnostic library) the pinned path if it fits, else generic."""
    if pin in (None, "slide") and slide_fits(L, level, H, W, C, nhwc):
        return "slide"
    if pin in (None, "fused") and fused_fits(L, level, W):
        return "fused"
    if pin in (None, "tiled") and plan_tiles(L, level, H, W):
        return "tiled"
    return "generic"


def workspace_bytes(L, level, H, W, C=3, pin=None, batch=B):
    """wv_swt2d_workspace_bytes: 3 fp32 planes per input plane when either layout ends in the generic kernels, else 0."""
    generic = "generic" in (path(L, level, H, W, C, False, pin), path(L, level, H, W, C, True, pin))
    return 3 * batch * C * H * W * 4 if generic else 0


# ------------------------------------------------------------------------------------------------ filters
def _made_up(L):
    """Fixed taps for counts no wavelet here has: a positive low-pass with sum |lo| = sqrt(2) like an orthogonal wavelet's,
    and a sign-alternating high-pass shifted to sum exactly 0 in fp64 and scaled to sum |hi| = sqrt(2) (one tap: hi = 0)."""
    m = np.arange(L, dtype=np.float64)
    lo = 1.0 + (7 * m) % 5
    hi = (-1.0) ** m * (1.0 + (3 * m) % 4)
    hi = hi - hi.mean()
    lo = lo / np.abs(lo).sum() * 2 ** 0.5
    hi = hi / max(np.abs(hi).sum(), 1e-300) * 2 ** 0.5
    return [float(v) for v in lo], [float(v) for v in hi]


MADE_UP = {"taps1": 1, "taps5": 5, "taps32": 32, "taps33": 33}
TAPS.update(MADE_UP)


def filters(name):
    """-> (dec_lo, dec_hi) lists of Python floats, for a wavelet name of oracle.swt_np or one of MADE_UP."""
    if name in MADE_UP:
        return _made_up(MADE_UP[name])
    from oracle import swt_np
    lo, hi = swt_np.WAVELETS[name]
    return list(lo), list(hi)


# ------------------------------------------------------------------------------------------------ case tables
WL = lambda L: NAME_OF_TAPS[L]
# a. tiled, pinned: every (taps, level) x its shapes; all KINDS x {f32, bf16} each.
#    36x132: two column tiles of 68, the second 4 columns short, and a partial row tile.
#    40x136 (level 3): (10, 3) gets TH = 8 at exactly 79,872 B = the two-per-CU limit; (8, 3) 70,656 B > 64 KiB, partial rows.
#    40x128 (level 3): the 161,952 B plan of (10, 3), TH = 28.  8x8: one tile smaller than its halo, wrapping several times.
TILED_SHAPES = {1: [(36, 132)], 2: [(36, 132)], 3: [(40, 136), (40, 128), (8, 8)]}
TILED_CASES = {(L, lev): [(WL(L), lev, H, W, 3) for H, W in TILED_SHAPES[lev]] for L in TILED_TAPS for lev in TILED_LEVELS}
TILED_224 = [("bior4.4", 3, 224, 224, 3), ("db4", 3, 224, 224, 3)]       # the workload's size; u8 NCHW -> f32 once
TILED_CHANNELS = [(wl, lev, 36, 132, C) for wl, lev in (("db2", 2), ("bior4.4", 1)) for C in (1, 2, 4)]
TILED_RELEASE = [("db4", 2, 40, 132, 3), ("bior4.4", 3, 40, 128, 3), ("bior4.4", 3, 40, 256, 3)]

# b. fused, pinned: every config x (wide tile partial in both axes, narrow tile with partial rows)
FUSED_CASES = {(L, lev): [(WL(L), lev) + ((40, 136) if lev == 3 else (36, 132)) + (3,), (WL(L), lev, 40, 128, 3)]
               for L, lev in CONFIGS}
FUSED_CHANNELS = [("db2", 3, 40, 136, C) for C in (1, 2, 4)] + [("db4", 1, 36, 132, C) for C in (1, 2, 4)]
#    release library, one row pair per config: wider than the sliding window (three wide tiles, the last partial; 264 where
#    level 3 needs W % 8 == 0) and narrower than it (H = 8 is below the window as well)
FUSED_RELEASE = {(L, lev): [(WL(L), lev, 8, 264 if lev == 3 else 260, 3), (WL(L), lev, 8, 32 if lev == 3 else 36, 3)]
                 for L, lev in CONFIGS}

# c. generic: (row, pin) with pin None = the release library ends there by itself, "generic" = WV_SWT_PATH=generic
GENERIC_CASES = [
    (("db2", 1, 30, 30, 3), None),             # W % 4 != 0
    (("haar", 2, 12, 20, 3), "generic"),       # W % 4 == 0: a fused shape, so pinned
    (("db2", 1, 6, 2, 3), None),               # W < taps: the wrap runs more than once
    (("taps5", 2, 24, 40, 3), None),
    (("taps32", 1, 16, 40, 3), None),
    (("taps1", 1, 8, 12, 3), None),
    (("haar", 4, 16, 48, 3), None),
    (("haar", 5, 32, 64, 3), None),
    (("db2", 4, 32, 48, 3), None),
    (("db2", 1, 30, 30, 1), None), (("taps5", 2, 24, 40, 2), None), (("haar", 4, 16, 48, 4), None),
]
REFUSED = ("taps33", 1, 16, 40, 3)                                        # WV_ENOTSUP
SHORT_WORKSPACE = ("db2", 1, 30, 30, 3)                                   # WV_ENOMEM
STRIDE_CASE = ("db2", 1, 420, 420, 3)                                     # B*C*H*W just above GRID_CAP; pinned generic


def all_rows():
    """Every row whose whole batch is compared with both references (the stride case checks three planes only)."""
    rows = [r for v in TILED_CASES.values() for r in v] + TILED_224 + TILED_CHANNELS + TILED_RELEASE
    rows += [r for v in FUSED_CASES.values() for r in v] + FUSED_CHANNELS + [r for v in FUSED_RELEASE.values() for r in v]
    rows += [r for r, _ in GENERIC_CASES]
    return sorted(set(rows))


# ------------------------------------------------------------------------------------------------ inputs and references
def seed_of(wl, lev, H, W, C):
    return 1000 * TAPS[wl] + 100 * lev + H + 7 * W + C


def images(wl, lev, H, W, C):
    """The row's uint8 [B, C, H, W] batch (swt_schedule_cases.noise: seeded, no two planes equal, read-only)."""
    return sc.noise(B, C, H, W, seed_of(wl, lev, H, W, C))


def device_input(x, kind):
    """swt_schedule_cases.device_input, plus NHWC for any channel count -> (GPU tensor, channels_last)."""
    assert kind in KINDS
    if x.shape[1] == 3 or not kind.endswith("nhwc"):
        return sc.device_input(x, kind)
    import torch
    t = torch.from_numpy(x.astype(np.float32) / np.float32(255.0) if kind.startswith("f32") else x.copy())
    return t.permute(0, 2, 3, 1).contiguous().cuda(), True


@functools.lru_cache(maxsize=4)
def reference(wl, lev, H, W, C):
    """C oracle of every plane of images(...): float32 [B, C, 4, H, W], read-only."""
    from oracle import swt_np
    out = swt_np.c_transform_planes(sc.unit_planes(images(wl, lev, H, W, C)), filters(wl), lev).reshape(B, C, 4, H, W)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def reference64(wl, lev, H, W, C):
    """The NumPy restatement in fp64 on the same fp32 pixels x / 255: float64 [B, C, 4, H, W], read-only."""
    from oracle import swt_np
    planes = sc.unit_planes(images(wl, lev, H, W, C))
    out = np.stack([swt_np.swt2_level_n(p, filters(wl), lev, dtype=np.float64) for p in planes]).reshape(B, C, 4, H, W)
    out.setflags(write=False)
    return out


def oracle_error(wl, lev, H, W, C):
    """max |C oracle - fp64| over the row's batch."""
    return float(np.abs(reference(wl, lev, H, W, C) - reference64(wl, lev, H, W, C)).max())
