"""No GPU: the case table of tests/hash_tail_cases.py keeps the conditions the GPU tests of the hashing tail rely on, route()
restates the dispatch of wv_hash_tail as written down by hand, and the host twin wv_hash_tail_cpu meets the same float64
reference, exact cases, pad-bit and sentinel checks as the kernels."""
import numpy as np
import pytest

import hash_tail_cases as tc

TWIN_POINTS = [pt for pt in tc.POINTS if pt[0] % 8 == 0]


def test_route_agrees_with_hand_written_expectations():
    expect = {(31, 384, None): "simple", (32, 384, None): "mfma", (64, 100, None): "valu16", (64, 504, "valu16"): "simple",
              (5, 384, "mfma"): "mfma", (65, 100, "mfma"): "valu16",
              (63, 100, None): "simple", (64, 500, None): "valu16", (64, 504, None): "simple", (1000, 504, "mfma"): "simple",
              (1, 32, "mfma"): "mfma", (1, 4, "mfma"): "simple", (4096, 384, "simple"): "simple", (4096, 384, "valu16"): "valu16",
              (63, 384, "valu16"): "simple", (64, 768, "valu16"): "simple", (32, 768, None): "mfma", (31, 768, None): "simple",
              (64, 416, "valu16"): "valu16", (40, 768, None): "mfma"}
    for (B, E, pin), kern in expect.items():
        assert tc.route(B, E, pin) == kern, (B, E, pin)
    # the LDS limit of the 16-sample kernel: 324 E bytes, 1 KB kept free of 160 KB
    assert 324 * 500 <= tc.MAX_LDS - 1024 < 324 * 504 and 324 * 203 > 64 * 1024 >= 324 * 202


def test_every_run_reaches_the_kernel_its_row_names():
    assert len(tc.POINTS) == len(tc.ES) + 2 * len(tc.NBITS) + len(tc.BS) - 2          # two points belong to two sweeps
    assert {E for E, _, _ in tc.POINTS} >= set(tc.ES) and {B for _, _, B in tc.POINTS} >= set(tc.BS)
    for E, n, B, pin, pset, kern in tc.RUNS:
        assert tc.route(B, E, pin) == kern, (E, n, B, pin)
    for kern in tc.KERNELS:                                      # every parameter set under every kernel
        assert {r[4] for r in tc.RUNS if r[5] == kern} == set(tc.SETS), kern


def test_random_cases_leave_under_one_percent_out_of_the_sign_check():
    worst = 0.0
    for E, n, B, pin, pset, kern in tc.RUNS:
        case = tc.random_case(E, n, B, pset)
        if pset in ("bn", "bias_bn"):
            g = case["bn_w"]
            assert (g > 0).any() or n == 1
            assert (g < 0).any() or n == 1
            assert (g == 0).sum() == (n > 1) and case["bn_var"].min() >= 0.5 and case["bn_var"].max() <= 2.0
        frac = tc.left_out(case)
        worst = max(worst, frac)
        assert frac < 0.01, (E, n, B, pset, frac)
    print(f"largest share left out of the sign check: {worst:.4%}")


def test_exact_cases_are_exactly_representable_and_hold_every_sign():
    seen = {s: set() for s in tc.SETS}
    for E, n, B, pin, pset, kern in tc.RUNS:
        for nonfinite in (True, False):
            case = tc.exact_case(E, n, B, pset, nonfinite)
            ref, _ = tc.reference(case)
            fin = np.isfinite(ref)
            assert np.array_equal(ref[fin].astype(np.float32).astype(np.float64), ref[fin])
            assert np.abs(ref[fin]).max() < 2 ** 24
            assert np.all(np.abs(case["x"][np.isfinite(case["x"])]) <= 3) and np.all(np.abs(case["w"]) <= 3)
            signs = set(np.sign(ref[fin]).tolist())
            seen[pset] |= signs
            if n >= 4:                                           # the built-in zero row and the +- pair
                assert signs == {-1.0, 0.0, 1.0}, (E, n, B, pset)
                assert np.all(ref[fin[:, 1], 1] == 0)
            if nonfinite and B >= 3:
                assert np.isnan(ref[B - 1]).all() and not np.isfinite(ref[B - 2]).any() and fin[:B - 2].all()
    assert all(s == {-1.0, 0.0, 1.0} for s in seen.values()), seen


@pytest.mark.parametrize("point", TWIN_POINTS, ids=lambda p: "E%d-n%d-B%d" % p)
def test_host_twin_against_float64_and_exact_cases(point):
    """wv_hash_tail_cpu at every point of the sweep it accepts (E % 8 == 0), each of the four parameter sets in turn: outputs
    fully written into pre-filled buffers, nothing behind them touched, pad bits 0, logits within the derived bound of the
    float64 reference, exact cases equal to it bit for bit; each subset of the outputs gives the same bits as all three."""
    E, n, B = point
    pset = tc.SETS[list(tc.POINTS).index(point) % 4]
    case = tc.random_case(E, n, B, pset)
    full = tc.run(case, "cpu")
    ratio = tc.check_random(case, full)
    print(f"hash_tail err/tol kernel=twin E={E} nbits={n} B={B} {pset}: {ratio:.4f}")
    for want in (("codes", "packed"), ("logits", "packed"), ("logits", "codes"), ("packed",)):
        part = tc.run(case, "cpu", want)
        assert tc.same_bits(part, {k: full[k] for k in want}), want
    exact = tc.exact_case(E, n, B, pset)
    out = tc.run(exact, "cpu")
    tc.check_exact(exact, out)
    calm = tc.run(tc.exact_case(E, n, B, pset, nonfinite=False), "cpu")
    keep = [b for b in range(B) if b not in (exact["nan_row"], exact["inf_row"])]
    assert tc.same_bits({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in calm.items()})


def test_host_twin_refusals():
    case = tc.random_case(100, 96, 65, "plain")
    rc, bufs = tc.call(case, "cpu")
    assert rc == tc.WV_EINVAL                                     # the twin needs E % 8 == 0
    fresh = tc.prefilled(65, 96)
    assert all(np.array_equal(bufs[k], fresh[k]) for k in fresh)
    case = tc.random_case(8, 96, 65, "bn")
    rc, bufs = tc.call(dict(case, bn_var=None), "cpu")
    assert rc == tc.WV_EINVAL
    rc, bufs = tc.call(case, "cpu", B=0)
    fresh = tc.prefilled(0, 96)
    assert rc == tc.WV_OK and all(np.array_equal(bufs[k], fresh[k]) for k in fresh)
