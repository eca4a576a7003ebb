"""The buffer-contract harness on the build machine (no GPU): the guard helper must be able to fail, every table row that
has a host twin runs that twin on guarded host memory -- same shapes, fills and placements as the GPU test -- against the
row's independent oracle, and the table must be complete (tests/buffer_contract_cases.py, tests/guarded.py)."""
import pytest
import torch

import buffer_contract_cases as BC
import group_layernorm_cases  # noqa: F401  (host margin below is test_host_group_layernorm.py's)
import ndcg_cases as NC_
from guarded import GUARD, GuardError, Guards, bits
from wvhash import _lib

GLN_MARGIN = 4.0            # test_host_group_layernorm.py: the twin's error against float64 <= 4 x stock F.layer_norm's


# ------------------------------------------------------------------------------------------ the helper can fail
def _set():
    g = Guards("cpu")
    a = g.place((5, 7), torch.int32, offset=4, fill=0xFF, name="lists")
    b = g.pitched(4, 5, 8, torch.float64, offset=8, fill=0x00, name="tables")
    c = g.place(33, torch.uint8, fill=0xFF, name="blob")
    return g, a, b, c


def test_untouched_buffers_pass_and_are_placed_as_asked():
    g, a, b, c = _set()
    assert a.data_ptr() % 256 == 4 and b.data_ptr() % 256 == 8 and c.data_ptr() % 256 == 0
    assert bool((a == -1).all()) and bool((b == 0).all()) and b.stride() == (8, 1) and bool((c == 255).all())
    a.fill_(3), b.fill_(1.5), c.fill_(9)                          # writing every payload byte is what outputs are for
    g.assert_intact()
    for p in g.placed:
        assert p.start >= GUARD and p.raw.numel() - (p.start + p.nbytes) == GUARD


@pytest.mark.parametrize("where,byte,names", [("behind", 5 * 7 * 4, ("lists", "back guard", "offset 140")),
                                              ("before", -1, ("lists", "front guard", "offset -1"))])
def test_a_byte_outside_the_payload_is_caught(where, byte, names):
    g, a, b, c = _set()
    p = g.placed[0]
    p.raw[p.start + byte] = 0
    with pytest.raises(GuardError) as e:
        g.assert_intact()
    assert all(n in str(e.value) for n in names), str(e.value)


def test_a_byte_in_a_pitch_gap_is_caught():
    g, a, b, c = _set()
    flat = torch.as_strided(b, (3 * 8 + 5,), (1,))
    flat[8 + 5] = 0.0                                             # row 1, first gap element: bytes 104.. of the payload
    with pytest.raises(GuardError) as e:
        g.assert_intact()
    assert "tables" in str(e.value) and "pitch gap of row 1" in str(e.value) and "offset 104" in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------ host twins under the harness
TWIN_ROWS = [r for r in BC.ROWS if r.twin is not None]


def _against_oracle(row, got, want):
    for o in row.outs:
        if o.name not in got:
            continue
        g, w = got[o.name], want[o.name]
        if o.check == "loss":
            continue
        if row.entry == "wv_group_layernorm":
            err = float((g.double() - w).abs().max())
            stock = float((want["stock"].to(o.dtype).double() - w).abs().max())
            print(f"{row.id}: twin {err:.3e} stock {stock:.3e}")
            assert err <= GLN_MARGIN * stock, (row.id, err, stock)
        elif o.dtype == torch.float64:                            # dcg / idcg: one sum of k terms each (ndcg_cases.sum_tol)
            for j, k in enumerate(row.ks):
                rel = ((g[:, j] - w[:, j]).abs() / w[:, j].abs().clamp(min=1e-300)).max()
                assert float(rel) <= NC_.sum_tol(k), (row.id, o.name, k, float(rel))
        elif o.dtype == torch.float32:                            # average precision
            assert float((g.double() - w.double()).abs().max()) <= BC.AP_TOL_ORACLE, (row.id, o.name)
        else:
            assert torch.equal(g.long(), w.long()), (row.id, o.name)
    if row.loss_check is not None:
        row.loss_check(got, want, row.id)


@pytest.mark.parametrize("row", TWIN_ROWS, ids=repr)
def test_host_twin_under_guards(row):
    lib = _lib.load()
    want = row.oracle()
    runs = {}
    for natural in (False, True):
        for fill in (0x00, 0xFF):
            runs[natural, fill] = got = BC.run_row(row, lib, "cpu", fill, natural=natural, host=True)
            _against_oracle(row, got, want)
    first = runs[False, 0x00]
    for key, got in runs.items():                                # no dependence on old content or on the placement
        for name in first:
            assert BC.same_bits(got[name], first[name]), (row.id, name, key)
    for o in row.outs:                                           # optional outputs of the twin
        if o.nullable and o.name in row.twin_outs:
            got = BC.run_row(row, lib, "cpu", 0xFF, null=(o.name,), host=True)
            for name in got:
                assert BC.same_bits(got[name], first[name]), (row.id, name, "without", o.name)


OPAQUE_ROWS = [r for r in BC.ROWS if (r.workspace is not None or r.blobs) and r.pin is None]


@pytest.mark.parametrize("row", OPAQUE_ROWS, ids=repr)
def test_a_misaligned_workspace_or_blob_is_refused_before_any_launch(row):
    """The refusal is host code that reads no pointer: checked here on host memory, and again on the GPU."""
    BC.run_refused(row, _lib.load(), "cpu")


# ------------------------------------------------------------------------------------------ table completeness
def test_every_entry_point_has_a_row():
    have = {r.entry for r in BC.ROWS}
    assert have == set(BC.ENTRY_POINTS), (have ^ set(BC.ENTRY_POINTS))
    assert all(hasattr(_lib.load(), e) for e in BC.ENTRY_POINTS)


def test_listed_shapes_reach_the_plans_they_are_listed_for():
    P = BC.rank_plan_of
    # Q = 17, N = 700: every pin of the lists, the windowed kernel alone for the fused modes
    for nbits in (64, 128):
        for k in BC.RANK_KS:
            assert P(17, 700, nbits, k, "lists", "0") == BC.Plan("column", 3, 0, True)
            assert P(17, 700, nbits, k, "lists", "64") == BC.Plan("window64", 11, 4, False)
            assert P(17, 700, nbits, k, "lists", "256") == P(17, 700, nbits, k, "lists", None) == BC.Plan("window256", 3, 4, False)
            assert P(17, 700, nbits, k, "ap", "0").kernel is None
        assert P(17, 700, nbits, 0, "radius", "64").kernel == "window256"
    u = BC.U32_COLUMN                                            # 65536 rows or more: the column kernel's 32-bit counters
    assert P(u["Q"], u["N"], u["nbits"], u["k"], "lists", None) == BC.Plan("column", 257, 0, False)
    for N, (C, NC) in BC.EDGES_256.items():
        assert P(3, N, 64, 37, "lists", "256") == BC.Plan("window256", C, NC, False), N
    for N, (C, NC) in BC.EDGES_64.items():
        assert P(3, N, 64, 37, "lists", "64") == BC.Plan("window64", C, NC, False), N
    # the edges are the first ragged database of an instantiation: one row fewer is the one below it
    assert [P(3, N - 1, 64, 37, "lists", "256").NC for N in (4097, 8193, 16385, 25601)] == [4, 8, 16, 25]
    assert [P(3, N - 1, 64, 37, "lists", "64").NC for N in (1025, 2049)] == [4, 8]
    assert {NC for r in BC.ROWS if r.plan for NC in [r.plan[-1].NC]} >= {4, 8, 16, 25, 32}
    # k = 37 over 17 rows: the distance rows start at every residue mod 16, the uint16 rows of odd queries at 2 mod 4
    assert {(q * 37) % 16 for q in range(17)} == set(range(16)) and {(q * 37 * 2) % 4 for q in range(17)} == {0, 2}
    for r in BC.ROWS:                                            # what every row's plan column says is what rank.hpp answers
        if r.plan:
            Q, N, nbits, k, mode, pin, plan = r.plan
            assert plan == P(Q, N, nbits, k, mode, pin) and plan.kernel is not None, r.id
            assert r.pin == pin
