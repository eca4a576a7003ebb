"""Shared by tests/test_swt_schedule_cases.py (no GPU) and tests/test_gpu_swt_schedule.py: the sliding SWT kernel's window
and plane schedule restated in plain Python (csrc/swt_slide.hip: slide_fits; csrc/swt_slide.hpp: slide_launch, PlaneSchedule),
the case tables that make a launch persistent on a device of `cu` compute units, seeded inputs in the five forms the
kernel reads, and the C oracle applied plane by plane.

The schedule: slide_launch starts grid = min(planes, 2 * cu) workgroups.  With 8 | grid (a persistent launch rounds the
grid down to that) image b belongs to XCD b % 8, whose planes are dealt in (image, channel) order to its grid / 8
workgroups, each looping q = wg_in_xcd, wg_in_xcd + grid / 8, ...; otherwise workgroup w takes planes w, w + grid, ....
"""
import functools

import numpy as np

TAPS = {"haar": 2, "db2": 4, "db4": 8, "bior4.4": 10}
TH = 16                 # rows per chunk (kSlideTH)
WGS_PER_CU = 2          # per_cu of slide_launch for every width the kernel takes
XCDS = 8
SHIPPED = [("haar", 1), ("db2", 3)]
OTHERS = [("haar", 2), ("haar", 3), ("db2", 1), ("db2", 2), ("db4", 1), ("bior4.4", 1)]
CUS = (32, 64, 256, 304)                                    # device sizes the case tables are checked for
KINDS = ("u8_planar", "u8_planar_off4", "u8_nhwc", "f32_planar", "f32_nhwc")
PLANAR_U8 = KINDS[:2]


def tol(level):
    """The bound of tests/test_gpu_swt.py: fused against separate multiply-add in fp32, values up to 2^level."""
    return 4e-6 * 2 ** level


def window(L, level):
    """-> halo, hmin, wmin of slide_fits (also: W % 4 == 0, W <= 256)."""
    halo = (L - 1) * ((1 << level) - 1)
    return halo, max(40, TH + 2 * halo), max(40, TH + halo)


def fits(wl, level, H, W):
    halo, hmin, wmin = window(TAPS[wl], level)
    return H >= hmin and wmin <= W <= 256 and W % 4 == 0 and H % (1 << level) == 0 and W % (1 << level) == 0


def nchunks(H, halo):
    """Chunks of TH rows the column cascade consumes per plane (H + halo rows)."""
    return (H + halo + TH - 1) // TH


def persistent_batch(cu, C, rem):
    """Smallest B with B % 8 == rem and B * C >= 2.3 * (2 * cu): every workgroup gets two or three planes."""
    B = -(-int(np.ceil(2.3 * WGS_PER_CU * cu)) // C)
    while B % 8 != rem:
        B += 1
    return B


def schedule(B, C, cu):
    """-> grid, nxcd, wg[B, C], it[B, C]: the workgroup that computes plane (b, c) and in which of its iterations."""
    planes, cap = B * C, WGS_PER_CU * cu
    grid, nxcd = min(planes, cap), XCDS
    if grid < planes:
        grid -= grid % nxcd
    if grid <= 0 or grid % nxcd:
        nxcd, grid = 1, min(planes, cap)
    per_xcd = grid // nxcd
    b, c = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    q = (b // nxcd) * C + c
    return grid, nxcd, (q % per_xcd) * nxcd + b % nxcd, q // per_xcd


def describe(bad, B, C, cu):
    """Flat plane numbers -> text naming (b, c), workgroup and iteration of the first few."""
    grid, nxcd, wg, it = schedule(B, C, cu)
    items = [f"(b={p // C}, c={p % C}: workgroup {wg[p // C, p % C]} iteration {it[p // C, p % C]})" for p in bad[:6]]
    return f"{len(bad)} of {B * C} planes, grid {grid}, nxcd {nxcd}: " + ", ".join(items)


# ------------------------------------------------------------------------------------------------ case tables
# a. the two shipped configs, persistent: (wavelet, level, H, W, C, rem, kinds).  Heights give both parities of nchunks (haar
#    level 1: 3, 4; db2 level 3: 6, 7); W = 40 has a partial last run and no coalesced producer, W = 48 the coalesced one.
def _shipped_cases():
    out = []
    for (wl, lev), (h0, h1) in zip(SHIPPED, ((40, 48), (64, 80))):
        out += [(wl, lev, h0, 40, 3, 0, KINDS), (wl, lev, h1, 48, 3, 5, KINDS),
                (wl, lev, h0, 48, 3, 5, ("u8_planar", "u8_nhwc")), (wl, lev, h1, 40, 3, 0, ("u8_planar", "u8_nhwc")),
                (wl, lev, h1, 40, 1, 4, PLANAR_U8), (wl, lev, h0, 48, 4, 3, PLANAR_U8)]
    return out


SHIPPED_CASES = _shipped_cases()
BF16_CASES = [("haar", 1, 48, 48, 3, 5), ("db2", 3, 64, 40, 3, 0)]      # shapes of SHIPPED_CASES; kinds below
BF16_KINDS = ("u8_planar", "f32_nhwc")
# b. the other six instantiations, persistent: C = 3, rem = 5, W = 48, one height per parity of nchunks
OTHER_CASES = [(wl, lev, H, 48, 3, 5, ("u8_planar", "u8_nhwc"))
               for wl, lev in OTHERS for H in ((40, 56) if (wl, lev) in (("db2", 2), ("bior4.4", 1)) else (40, 48))]
# c. few planes: (B, C) -> nxcd the launch must choose
FEW_SHAPES = [("haar", 1, 40, 48), ("db2", 3, 64, 48)]
FEW_PLANES = {(4, 4): 8, (1, 8): 8, (8, 1): 8, (16, 1): 8, (8, 3): 8, (3, 8): 8, (9, 8): 8, (12, 2): 8, (5, 3): 1, (7, 1): 1}
# d. band-major into a padded buffer shared by two calls
SPLIT_B, SPLIT_B0, SPLIT_C, SPLIT_PAD = 8, 3, 3, 64


def flat(cases):
    """(wl, lev, H, W, C, rem, kinds) rows -> one (wl, lev, H, W, C, rem, kind) per kind, rows of one shape adjacent."""
    return [row[:6] + (k,) for row in cases for k in row[6]]


# ------------------------------------------------------------------------------------------------ inputs and reference
@functools.lru_cache(maxsize=2)
def noise(B, C, H, W, seed):
    """uint8 [B, C, H, W]; the first two pixels of a plane hold its number, so no two planes are equal."""
    x = np.random.default_rng(seed).integers(0, 256, size=(B, C, H, W), dtype=np.uint8)
    p = np.arange(B * C).reshape(B, C)
    x[:, :, 0, 0], x[:, :, 0, 1] = p & 255, p >> 8
    x.setflags(write=False)
    return x


def unit_planes(x):
    """[B, C, H, W] uint8 -> [B*C, H, W] float32 x / 255 (IEEE division, what the kernel's conversion equals)."""
    return (x.astype(np.float32) / np.float32(255.0)).reshape((-1,) + x.shape[2:])


def device_input(x, kind):
    """-> (GPU tensor in the form `kind`, channels_last).  Slices along the batch keep the form."""
    import torch
    B, C = x.shape[:2]
    assert kind in KINDS and (C == 3 or not kind.endswith("nhwc"))
    if kind.startswith("f32"):
        t = torch.from_numpy(x.astype(np.float32) / np.float32(255.0))
    else:
        t = torch.from_numpy(x.copy())
    if kind.endswith("nhwc"):
        return t.permute(0, 2, 3, 1).contiguous().cuda(), True
    if kind == "u8_planar_off4":
        buf = torch.empty(t.numel() + 16, dtype=torch.uint8, device="cuda")
        view = buf[4:4 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view, False
    t = t.cuda()
    assert t.data_ptr() % 16 == 0
    return t, False


@functools.lru_cache(maxsize=1)
def reference(wl, lev, B, C, H, W, seed):
    """C oracle of every plane of noise(...): float32 [B, C, 4, H, W]."""
    from oracle import swt_np
    return swt_np.c_transform_planes(unit_planes(noise(B, C, H, W, seed)), wl, lev).reshape(B, C, 4, H, W)


def seed_of(wl, lev, H, W, C):
    return 1000 * TAPS[wl] + 100 * lev + H + 7 * W + C
