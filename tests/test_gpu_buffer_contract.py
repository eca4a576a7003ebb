"""Where the retrieval and loss entry points write and what they read: every row of tests/buffer_contract_cases.py through
the C ABI on guarded device memory (tests/guarded.py).  Expected bits come from the host twins, never from a second GPU call.

Per row, in this order:
  1. aligned placement, payloads pre-filled 0x00 and 0xFF: rc == 0, outputs equal the expected bits under both fills (fully
     written, no dependence on old content -- the workspace of exactly the reported bytes and the prepared blobs included),
     results equal across the fills bit for bit, guards and pitch gaps intact, inputs unchanged;
  2. natural placement (every output one element past a 256-byte boundary; the inputs whose alignment picks a path moved
     too: db of wv_ip_map_at_k at 4 mod 16, dist_matrix of wv_rank_from_dist at 1 mod 16, x of wv_group_layernorm by one
     element, db of wv_db_prepare / wv_hamming_dist at 8 mod 16 -- a row slice of 64-bit codes, which the tile loads of
     csrc/hamming.hip read 16 bytes at a time without a test until they were given the 8-byte path): the same assertions,
     and the results of step 1 bit for bit.  Every access of these kernels to a moved buffer is
     either no wider than the element or guarded by a run-time alignment test (rank2_copy_list, rank2_dist_row, the column
     kernel's `aligned`, wv_ip_map_at_k's `vec`, wv_group_layernorm's `wide`, wv_hamming_dist_prepared's `aligned`);
     workspaces and prepared blobs are opaque bytes read with 16-byte loads and stay 256-byte aligned, as include/wvhash.h
     now requires;
  3. optional outputs (dist, cum, nrel, grad) passed as NULL one at a time and all together: the rest bit for bit.
Loss values are held to the twin within TOL (C.check) and to themselves bit for bit across fills and placements."""
import itertools

import pytest
import torch

import buffer_contract_cases as BC
from wvhash import _lib

pytestmark = pytest.mark.gpu


def _against_expected(row, got, want):
    for o in row.outs:
        if o.name not in got:
            continue
        g, w = got[o.name], want[o.name]
        if o.check == "bits":
            if not BC.same_bits(g, w):
                bad = (BC.bits(g) != BC.bits(w)).nonzero()
                raise AssertionError(f"{row.id}: output {o.name} differs from the twin's bits at byte {int(bad[0])} "
                                     f"({bad.numel()} bytes of {BC.bits(w).numel()})")
        elif o.check == "ap":
            err = float((g - w).abs().max())
            print(f"{row.id}: one wave per query, AP against the twin {err:.3e}")
            assert err <= BC.AP_TOL_ONE_WAVE, (row.id, err)
    if row.loss_check is not None:
        row.loss_check(got, want, row.id)


@pytest.mark.parametrize("row", BC.ROWS, ids=repr)
def test_buffer_contract(row, request):
    if row.pin is not None:
        request.getfixturevalue("diag").setenv("WV_TOPK_V2", row.pin)
    lib = _lib.require_gpu()
    torch.cuda.set_device(0)
    want = {fill: row.expected(lib, fill) for fill in (0x00, 0xFF)}
    runs = {}
    for natural in (False, True):                                 # steps 1 and 2
        for fill in (0x00, 0xFF):
            runs[natural, fill] = got = BC.run_row(row, lib, "cuda", fill, natural=natural)
            _against_expected(row, got, want[fill])
    first = runs[False, 0x00]
    for key, got in runs.items():
        for name in first:
            if name != "wire":                                    # a wire buffer's unowned words hold the fill
                assert BC.same_bits(got[name], first[name]), (row.id, name, key)
    optional = [o.name for o in row.outs if o.nullable]           # step 3
    nulls = [(n,) for n in optional] + ([tuple(optional)] if len(optional) > 1 else [])
    for null, natural in itertools.product(nulls, (False, True)):
        got = BC.run_row(row, lib, "cuda", 0xFF, natural=natural, null=null)
        assert set(got) == set(first) - set(null)
        for name in got:
            assert BC.same_bits(got[name], first[name]), (row.id, name, "without", null, natural)


@pytest.mark.parametrize("row", [r for r in BC.ROWS if r.workspace is not None or r.blobs], ids=repr)
def test_misaligned_workspace_or_blob_is_refused_untouched(row, request):
    """Workspaces and prepared blobs are read 16 bytes at a time and carry no run-time test in the kernels: 8 bytes past a
    16-byte boundary the entry point answers WV_EINVAL before any launch and every buffer keeps its bytes."""
    if row.pin is not None:
        request.getfixturevalue("diag").setenv("WV_TOPK_V2", row.pin)
    BC.run_refused(row, _lib.require_gpu(), "cuda")
