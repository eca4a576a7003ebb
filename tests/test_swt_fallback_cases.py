"""The case tables of tests/swt_fallback_cases.py do what tests/test_gpu_swt_fallback.py relies on (no GPU needed): every
row reaches the implementation and the tile edge it is listed for -- by the planner of csrc/swt.hip restated in Python --
every template instantiation of the fused and the tiled kernel has a row, and the C oracle alone stays within a quarter
of the GPU bound of the fp64 restatement on every row."""
import numpy as np
import pytest

import swt_fallback_cases as fc


def taps_level(row):
    return fc.TAPS[row[0]], row[1]


def test_restated_planner_on_known_plans():
    # LDS of the tiled kernel: the figures of csrc/swt.hip's plan for bior4.4 level 3
    assert fc.plan_tiles(10, 3, 224, 224)["lds"] == 156960
    for W in (128, 256, 512):
        p = fc.plan_tiles(10, 3, 224, W)
        assert (p["TH"], p["TW"], p["lds"]) == (28, 128, 161952) and fc.MAX_LDS - 1024 - p["lds"] == 864
    assert fc.plan_tiles(4, 3, 224, 224)["TW"] == 112 and fc.plan_tiles(2, 1, 30, 30) is None
    assert fc.plan_tiles(6, 1, 32, 32) is None and fc.plan_tiles(2, 4, 32, 32) is None
    # fused tile choice: 224 and its multiples wide, powers of two narrow
    assert fc.fused_plan(224, 224)["kind"] == "wide" and fc.fused_plan(64, 256)["kind"] == "narrow"
    assert fc.fused_fits(4, 3, 8) and not fc.fused_fits(8, 2, 64) and not fc.fused_fits(4, 3, 30)
    # choose(): the shapes tests/test_gpu_cabi.py pins, and the release choice of tests/test_gpu_swt.py's edge cases
    assert fc.path(4, 3, 224, 224) == "slide" and fc.path(4, 3, 48, 224) == "fused" and fc.path(4, 3, 512, 384) == "fused"
    assert fc.path(4, 3, 48, 224, pin="slide") == "generic" and fc.path(4, 3, 64, 96, pin="slide") == "slide"
    assert fc.path(4, 3, 64, 96, C=4, nhwc=True) == "fused" and fc.path(8, 2, 96, 96) == "tiled"
    assert fc.path(10, 2, 64, 32) == "tiled" and fc.path(8, 3, 32, 32) == "tiled" and fc.path(6, 2, 32, 32) == "generic"
    assert fc.workspace_bytes(4, 3, 48, 224, pin="slide") == 3 * 2 * 3 * 48 * 224 * 4
    assert fc.workspace_bytes(4, 3, 64, 96, C=4, pin="slide") == 3 * 2 * 4 * 64 * 96 * 4      # NHWC with C != 3 falls back
    assert fc.workspace_bytes(4, 3, 224, 224, pin="tiled") == 0 == fc.workspace_bytes(2, 1, 224, 224, pin="fused")


def test_every_row_is_a_valid_small_shape():
    rows = fc.all_rows() + [fc.REFUSED, fc.SHORT_WORKSPACE, fc.STRIDE_CASE]
    for wl, lev, H, W, C in rows:
        assert H % 2 ** lev == 0 and W % 2 ** lev == 0 and 1 <= lev <= 5 and C in (1, 2, 3, 4), (wl, lev, H, W, C)
        assert H <= 420 and W <= 420 and len(fc.filters(wl)[0]) == len(fc.filters(wl)[1]) == fc.TAPS[wl]
    big = [r for r in fc.all_rows() if r[2] * r[3] > 40 * 264]
    assert sorted(big) == sorted(fc.TILED_224)                  # everything else is a few thousand pixels


def test_tiled_rows_hit_their_edges():
    assert set(fc.TILED_CASES) == {(L, n) for L in (2, 4, 8, 10) for n in (1, 2, 3)} and len(fc.TILED_CASES) == 12
    for (L, lev), rows in fc.TILED_CASES.items():
        assert all(taps_level(r) == (L, lev) and r[4] == 3 for r in rows)
        plans = {r[2:4]: fc.plan_tiles(L, lev, r[2], r[3]) for r in rows}
        assert all(plans.values()) and all(fc.path(L, lev, H, W, pin="tiled") == "tiled" for H, W in plans)
        if lev < 3:
            p = plans[(36, 132)]                                # two column tiles, the last 4 short, and a partial row tile
            assert (p["TW"], p["tilesX"], p["last_w"]) == (68, 2, 64) and p["tilesY"] == 2 and 0 < p["last_h"] < p["TH"]
        else:
            assert set(plans) == {(40, 136), (40, 128), (8, 8)}
            p = plans[(40, 136)]                                # more than one column tile together with a partial row tile
            assert (p["TW"], p["tilesX"]) == (68, 2) and p["tilesY"] >= 2
            assert plans[(40, 128)]["tilesX"] == 1 and plans[(40, 128)]["TW"] == 128
            p = plans[(8, 8)]                                   # one tile, smaller than the halo it wraps around itself
            assert (p["TH"], p["TW"], p["tilesX"], p["tilesY"]) == (8, 8, 1, 1) and p["halo_rows"] >= (8 if L > 2 else 7)
    p = fc.plan_tiles(10, 3, 40, 136)
    assert (p["TH"], p["lds"]) == (8, 79872) and p["lds"] == fc.TWO_PER_CU and p["tilesY"] == 5
    p = fc.plan_tiles(8, 3, 40, 136)
    assert p["lds"] == 70656 and p["lds"] > 64 * 1024 and 0 < p["last_h"] < p["TH"]
    p = fc.plan_tiles(10, 3, 40, 128)                           # the largest LDS request the planner can make
    assert (p["TH"], p["lds"], p["tilesY"], p["last_h"]) == (28, 161952, 2, 12) and p["lds"] > 64 * 1024
    assert max(fc.plan_tiles(L, n, H, W)["lds"] for L in (2, 4, 8, 10) for n in (1, 2, 3)
               for H in (8, 32, 40, 224) for W in range(4, 516, 4) if fc.plan_tiles(L, n, H, W)) == 161952
    # both sides of the 64 KiB switch (hipFuncSetAttribute) occur
    sizes = [fc.plan_tiles(*taps_level(r), r[2], r[3])["lds"] for rows in fc.TILED_CASES.values() for r in rows]
    assert min(sizes) < 64 * 1024 < max(sizes)
    assert [taps_level(r) for r in fc.TILED_224] == [(10, 3), (8, 3)] and all(r[2:] == (224, 224, 3) for r in fc.TILED_224)
    assert fc.plan_tiles(10, 3, 224, 224)["lds"] == 156960 and fc.plan_tiles(8, 3, 224, 224)["lds"] > 64 * 1024
    assert {(taps_level(r), r[4]) for r in fc.TILED_CHANNELS} == {(tl, C) for tl in ((4, 2), (10, 1)) for C in (1, 2, 4)}
    assert all(r[2:4] == (36, 132) and fc.path(*taps_level(r), 36, 132, r[4], True, "tiled") == "tiled" for r in fc.TILED_CHANNELS)


def test_tiled_release_rows_reach_the_tiled_kernel_unpinned():
    assert fc.TILED_RELEASE == [("db4", 2, 40, 132, 3), ("bior4.4", 3, 40, 128, 3), ("bior4.4", 3, 40, 256, 3)]
    for wl, lev, H, W, C in fc.TILED_RELEASE:
        L = fc.TAPS[wl]
        for nhwc in (False, True):
            assert fc.path(L, lev, H, W, C, nhwc) == "tiled" and not fc.swt_config(L, lev)
        assert fc.workspace_bytes(L, lev, H, W, C) == 0
    assert fc.sc.window(10, 1)[2] <= 256 and fc.sc.fits("bior4.4", 1, 40, 256)      # W = 256: level 1 would slide ...
    assert not fc.slide_fits(10, 3, 40, 256)                                        # ... (10, 3) is no sliding config
    assert fc.plan_tiles(10, 3, 40, 256)["tilesX"] == 2 and fc.plan_tiles(10, 3, 40, 256)["lds"] == 161952


def test_fused_rows_hit_their_edges():
    assert set(fc.FUSED_CASES) == set(fc.CONFIGS) == set(fc.FUSED_RELEASE) and len(fc.CONFIGS) == 8
    for (L, lev), rows in fc.FUSED_CASES.items():
        assert all(taps_level(r) == (L, lev) and r[4] == 3 for r in rows) and len(rows) == 2
        assert all(fc.path(L, lev, r[2], r[3], pin="fused") == "fused" for r in rows)
        wide, narrow = (fc.fused_plan(r[2], r[3]) for r in rows)
        assert wide["kind"] == "wide" and wide["tilesX"] == 2 and 0 < wide["last_w"] < 112 and 0 < wide["last_h"] < 32
        assert rows[1][2:4] == (40, 128) and narrow["kind"] == "narrow" and narrow["tilesX"] == 2 and narrow["last_w"] == 64
        assert narrow["tilesY"] == 2 and narrow["last_h"] == 8
    assert {(taps_level(r), r[4]) for r in fc.FUSED_CHANNELS} == {(tl, C) for tl in ((4, 3), (8, 1)) for C in (1, 2, 4)}
    assert all(fc.path(*taps_level(r), r[2], r[3], r[4], True, "fused") == "fused" for r in fc.FUSED_CHANNELS)
    for (L, lev), (big, small) in fc.FUSED_RELEASE.items():
        for wl, n, H, W, C in (big, small):
            assert (fc.TAPS[wl], n) == (L, lev)
            for nhwc in (False, True):                          # the release library gets there by itself
                assert not fc.slide_fits(L, lev, H, W, C, nhwc) and fc.path(L, lev, H, W, C, nhwc) == "fused"
        p = fc.fused_plan(*big[2:4])
        assert big[3] > 256 and p["kind"] == "wide" and p["tilesX"] == 3 and 0 < p["last_w"] < 112
        assert small[3] < fc.sc.window(L, lev)[2] and fc.fused_plan(*small[2:4])["tilesX"] == 1


def test_generic_rows_reach_the_generic_kernels():
    for (wl, lev, H, W, C), pin in fc.GENERIC_CASES:
        L = fc.TAPS[wl]
        release = {fc.path(L, lev, H, W, C, nhwc) for nhwc in (False, True)}
        assert (release == {"generic"}) == (pin is None), (wl, lev, H, W)           # pinned exactly where it has to be
        assert fc.path(L, lev, H, W, C, pin=pin) == "generic"
        assert fc.workspace_bytes(L, lev, H, W, C, pin) == 3 * fc.B * C * H * W * 4
    rows = [r for r, _ in fc.GENERIC_CASES]
    assert {r[3] % 4 for r in rows} == {0, 2} and ("db2", 1, 6, 2, 3) in rows        # W % 4 != 0; W smaller than the taps
    assert {fc.TAPS[r[0]] for r in rows} >= {1, 2, 4, 5, 32} and {r[1] for r in rows} >= {1, 2, 4, 5}
    assert {r[4] for r in rows} == {1, 2, 3, 4}
    for name, L in fc.MADE_UP.items():
        lo, hi = fc.filters(name)
        assert len(lo) == L and abs(sum(hi)) < 1e-15 and abs(sum(abs(v) for v in lo) - 2 ** 0.5) < 1e-12
    assert fc.TAPS[fc.REFUSED[0]] == 33 and fc.TAPS["taps32"] == 32
    assert fc.path(4, 1, 30, 30) == "generic" and fc.SHORT_WORKSPACE == ("db2", 1, 30, 30, 3)
    wl, lev, H, W, C = fc.STRIDE_CASE
    n = fc.B * C * H * W
    assert fc.GRID_CAP < n < 2 * fc.GRID_CAP and n - fc.GRID_CAP < H * W and max(H, W) <= 420
    assert fc.GRID_CAP // (H * W) == fc.B * C - 1               # the plane straddling the second turn is the last one
    assert fc.path(4, 1, H, W) == "fused" and fc.path(4, 1, H, W, pin="generic") == "generic"
    assert max(fc.B * r[4] * r[2] * r[3] for r in fc.all_rows()) < fc.GRID_CAP       # no other row takes a second turn


def test_every_instantiation_has_a_row():
    """32 fused kernels = 8 configs x {u8, f32} x {wide, narrow}; 48 tiled = 12 (taps, level) x {u8, f32} x {f32, bf16}.
    The GPU tests run all four input forms and both output types on every row of the two pinned tables."""
    fused = {(tl, fc.fused_plan(r[2], r[3])["kind"], kind[:3]) for tl, rows in fc.FUSED_CASES.items() for r in rows
             for kind in fc.KINDS}
    assert len(fused) == 32
    tiled = {(tl, kind[:3], out) for tl in fc.TILED_CASES for kind in fc.KINDS for out in ("f32", "bf16")}
    assert len(tiled) == 48
    assert {k[:3] for k in fc.KINDS} == {"u8_", "f32"} and {k.endswith("nhwc") for k in fc.KINDS} == {False, True}


@pytest.mark.parametrize("row", fc.all_rows(), ids=lambda r: "-".join(map(str, r)))
def test_c_oracle_is_within_a_quarter_of_the_bound_of_fp64(row):
    wl, lev, H, W, C = row
    ref = fc.reference(*row)
    assert ref.shape == (fc.B, C, 4, H, W) and ref.dtype == np.float32 and np.isfinite(ref).all()
    err = fc.oracle_error(*row)
    print(f"{wl} L{lev} {H}x{W} C={C}: max |C oracle - fp64| = {err:.3e} = {err / fc.tol(lev):.3f} of the bound")
    assert err <= 0.25 * fc.tol(lev)


def test_inputs_are_kept_and_distinct():
    x = fc.images("db2", 2, 36, 132, 4)
    assert x.shape == (2, 4, 36, 132) and x.dtype == np.uint8 and not x.flags.writeable
    assert len({p.tobytes() for p in x.reshape(8, -1)}) == 8 and fc.images("db2", 2, 36, 132, 4) is x
    assert not fc.reference("db2", 2, 36, 132, 4).flags.writeable
