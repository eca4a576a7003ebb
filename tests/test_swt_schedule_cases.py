"""The case tables of tests/swt_schedule_cases.py do what tests/test_gpu_swt_schedule.py relies on (no GPU needed): every
shape lies in the sliding kernel's window, both parities of the chunk count occur for every (taps, level), the batches make
the launch persistent with two or three planes per workgroup and unequal XCD shares on devices of 32 to 304 compute units,
the few-plane cases get the XCD mapping the table says, and the outputs stay small.  And the per-plane C oracle is the
batch oracle."""
import numpy as np
import pytest

import swt_schedule_cases as sc
from oracle import swt_np
from wvhash import synth

PERSISTENT = sc.SHIPPED_CASES + sc.OTHER_CASES


def test_every_shape_is_inside_the_window():
    shapes = [row[:4] for row in PERSISTENT] + sc.FEW_SHAPES + [row[:4] for row in sc.BF16_CASES]
    for wl, lev, H, W in shapes:
        halo, hmin, wmin = sc.window(sc.TAPS[wl], lev)
        assert halo == (sc.TAPS[wl] - 1) * (2 ** lev - 1) and hmin == max(40, 16 + 2 * halo) and wmin == max(40, 16 + halo)
        assert H >= hmin and wmin <= W <= 256 and W % 4 == 0 and H % 2 ** lev == 0 and W % 2 ** lev == 0, (wl, lev, H, W)
        assert sc.fits(wl, lev, H, W)
    assert not sc.fits("db2", 3, 56, 48) and not sc.fits("haar", 1, 40, 36) and not sc.fits("haar", 1, 40, 42)
    assert not sc.fits("haar", 1, 40, 260) and not sc.fits("haar", 3, 44, 48)


def test_tables_hold_what_they_should():
    assert {row[:2] for row in sc.SHIPPED_CASES} == set(sc.SHIPPED) and {row[:2] for row in sc.OTHER_CASES} == set(sc.OTHERS)
    for cfg, heights, chunks in ((("haar", 1), {40, 48}, {3, 4}), (("db2", 3), {64, 80}, {6, 7})):
        rows = [r for r in sc.SHIPPED_CASES if r[:2] == cfg]
        halo = sc.window(sc.TAPS[cfg[0]], cfg[1])[0]
        assert {r[2] for r in rows} == heights and {sc.nchunks(r[2], halo) for r in rows} == chunks
        assert {r[3] for r in rows} == {40, 48} and {r[4:6] for r in rows} == {(3, 0), (3, 5), (1, 4), (4, 3)}
        assert {k for r in rows for k in r[6]} == set(sc.KINDS)
        for r in rows:
            assert set(r[6]) <= set(sc.KINDS if r[4] == 3 else sc.PLANAR_U8)
        # every height, width and input kind also meets both producers' widths / both parities
        assert {(r[2], r[3]) for r in rows} == {(h, w) for h in heights for w in (40, 48)}
        for kind in sc.KINDS:
            assert {sc.nchunks(r[2], halo) % 2 for r in rows if kind in r[6]} == {0, 1}, kind
    for row in sc.BF16_CASES:
        assert any(r[:6] == row and set(sc.BF16_KINDS) <= set(r[6]) for r in sc.SHIPPED_CASES)
    assert {row[:2] for row in sc.BF16_CASES} == set(sc.SHIPPED)
    for r in sc.OTHER_CASES:
        assert r[3:] == (48, 3, 5, ("u8_planar", "u8_nhwc"))
    flat = sc.flat(PERSISTENT)
    assert len(flat) == sum(len(r[6]) for r in PERSISTENT) and len(set(flat)) == len(flat)


def test_both_chunk_parities_for_every_taps_and_level():
    seen = {}
    for wl, lev, H, *_ in PERSISTENT:
        seen.setdefault((wl, lev), set()).add(sc.nchunks(H, sc.window(sc.TAPS[wl], lev)[0]) % 2)
    assert set(seen) == set(sc.SHIPPED + sc.OTHERS)
    assert all(p == {0, 1} for p in seen.values()), seen
    assert sc.nchunks(40, 1) == 3 and sc.nchunks(48, 1) == 4 and sc.nchunks(64, 21) == 6 and sc.nchunks(80, 21) == 7
    assert sc.nchunks(224, 21) == 16                        # the one persistent shape of tests/test_gpu_swt.py: even


@pytest.mark.parametrize("cu", sc.CUS)
def test_batches_make_the_launch_persistent(cu):
    for wl, lev, H, W, C, rem, _ in PERSISTENT:
        B = sc.persistent_batch(cu, C, rem)
        assert B % 8 == rem and B * C >= 2.3 * (2 * cu) and B * C > 2 * (2 * cu)
        assert (B - 8) * C < 2.3 * (2 * cu)                                     # the smallest such B
        grid, nxcd, wg, it = sc.schedule(B, C, cu)
        assert nxcd == 8 and grid == 2 * cu - 2 * cu % 8 and grid < B * C
        per_wg = np.bincount(wg.ravel(), minlength=grid)
        assert per_wg.min() >= 2 and per_wg.max() <= 3, (cu, C, rem, per_wg.min(), per_wg.max())
        assert sorted(set(it.ravel())) == list(range(per_wg.max()))
        # a plane is computed exactly once: (workgroup, iteration) pairs are distinct
        assert len(set(zip(wg.ravel().tolist(), it.ravel().tolist()))) == B * C
        share = np.bincount(np.arange(B) % 8, minlength=8) * C                  # planes per XCD
        assert (share.max() != share.min()) == (rem != 0)
        if cu == 256:
            assert B * C * 4 * H * W * 4 <= 128 * 2 ** 20, (wl, lev, H, W, B, C)
    assert sc.persistent_batch(256, 3, 0) == 400 and sc.persistent_batch(256, 3, 5) == 397
    assert sc.persistent_batch(256, 1, 4) == 1180 and sc.persistent_batch(256, 4, 3) == 299


@pytest.mark.parametrize("cu", sc.CUS)
def test_few_plane_cases_get_the_listed_xcd_mapping(cu):
    assert len(sc.FEW_PLANES) == 10
    for (B, C), want in sc.FEW_PLANES.items():
        grid, nxcd, wg, it = sc.schedule(B, C, cu)
        assert nxcd == want and (B * C % 8 == 0) == (want == 8), (B, C)
        assert grid == min(B * C, 2 * cu) and (cu < 64 or grid == B * C)        # from 64 CUs on: B * C workgroups
        assert len(set(zip(wg.ravel().tolist(), it.ravel().tolist()))) == B * C and wg.max() < grid
        if want == 8:
            assert np.array_equal(wg % 8, np.repeat((np.arange(B) % 8)[:, None], C, axis=1))   # image b on XCD b % 8
        else:
            assert (it == 0).all() and np.array_equal(wg.ravel(), np.arange(B * C))
    # the example of the issue: B = 4, C = 4 leaves XCDs 4-7 empty and gives the workgroups of XCDs 0-3 two planes each
    grid, nxcd, wg, it = sc.schedule(4, 4, 256)
    assert np.array_equal(np.bincount(wg.ravel(), minlength=16), [2, 2, 2, 2, 0, 0, 0, 0] * 2) and it.max() == 1


def test_split_case_shape():
    B, b0, C = sc.SPLIT_B, sc.SPLIT_B0, sc.SPLIT_C
    assert (B, b0, C, sc.SPLIT_PAD) == (8, 3, 3, 64)
    assert sc.schedule(B, C, 256)[1] == 8 and sc.schedule(b0, C, 256)[1] == 1 and sc.schedule(B - b0, C, 256)[1] == 1


def test_noise_planes_are_distinct_and_kept():
    x = sc.noise(13, 4, 40, 48, seed=5)
    assert x.dtype == np.uint8 and x.shape == (13, 4, 40, 48) and not x.flags.writeable
    assert len({p.tobytes() for p in x.reshape(-1, 40 * 48)}) == 52
    assert sc.noise(13, 4, 40, 48, seed=5) is x
    y = sc.noise(1180, 1, 40, 40, seed=6)
    assert len({bytes(p[0, :2]) for p in y.reshape(-1, 40, 40)}) == 1180
    u = sc.unit_planes(x)
    assert u.dtype == np.float32 and u.shape == (52, 40, 48) and u.max() <= 1.0
    assert np.array_equal(u[5], x[1, 1].astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("wl,lev", [("haar", 1), ("db2", 3), ("bior4.4", 1)])
def test_plane_oracle_equals_batch_oracle_bit_for_bit(wl, lev):
    img = synth.noise_images(3, 64, 48, seed=9)                                  # [B, H, W, 3] uint8
    batch = swt_np.c_transform_batch(img, wl, lev)
    planes = swt_np.c_transform_planes(sc.unit_planes(np.ascontiguousarray(img.transpose(0, 3, 1, 2))), wl, lev)
    assert planes.shape == (9, 4, 64, 48) and planes.dtype == np.float32
    assert np.array_equal(planes.reshape(3, 3, 4, 64, 48), batch)
