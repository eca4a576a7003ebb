"""The three kernels behind wv_hash_tail (csrc/head.hip: k_hash_tail, k_hash_tail16, k_hash_tail_mfma) against a float64
evaluation with a derived per-element bound, and against exactly representable cases where no rounding can hide a dropped or
doubled term -- at the widths, code lengths and batch sizes where each kernel takes another path (tests/hash_tail_cases.py).

Every run names the kernel it must reach and holds that against route(), the dispatch rule restated in Python.  Which kernel
really ran cannot be observed from here, so behaviour stands in for it: a pin that route() says falls through to a chain
kernel gives the bits of the `simple` pin, and the matrix-core kernel (another summation order) differs from the chain in at
least one bit on random data.  `valu16` and `simple` are the same fmaf chain and cannot be told apart this way: for those
two the tests rely on route() alone.
"""
import numpy as np
import pytest
import torch

import hash_tail_cases as tc

pytestmark = pytest.mark.gpu

RUN = pytest.mark.parametrize("run", tc.RUNS, ids=tc.run_id)
POINT = pytest.mark.parametrize("point", list(tc.POINTS), ids=lambda p: "E%d-n%d-B%d" % p)
SUBSETS = (("codes", "packed"), ("logits", "packed"), ("logits", "codes"), ("packed",))     # the last: what encode_packed asks for


def pinned(diag, pin):
    if pin is None:
        diag.delenv("WV_HASH_TAIL", raising=False)
    else:
        diag.setenv("WV_HASH_TAIL", pin)


@RUN
def test_random_case_against_float64_with_every_output_written(run, diag):
    """Outputs pre-filled (NaN, 0xA5 bytes) in front of a 4 KB sentinel: every element is written, the pad bits above nbits are
    0, nothing behind the outputs is touched; logits within the derived bound of the float64 reference, codes and bits those of
    the reference wherever it is further than the bound from zero, and everywhere those of the kernel's own logits.  With any
    output pointer NULL, and with only `packed` asked for, what remains is the same bit for bit."""
    E, n, B, pin, pset, kern = run
    assert tc.route(B, E, pin) == kern
    pinned(diag, pin)
    case = tc.random_case(E, n, B, pset)
    full = tc.run(case, "gpu")
    ratio = tc.check_random(case, full)
    print(f"hash_tail err/tol kernel={kern} pin={pin} E={E} nbits={n} B={B} {pset}: {ratio:.4f}")
    for want in SUBSETS:
        part = tc.run(case, "gpu", want)
        assert tc.same_bits(part, {k: full[k] for k in want}), want


@RUN
def test_exact_case_is_bit_equal_to_float64(run, diag):
    """Integer inputs: the logits equal the float64 reference bit for bit.  A logit of exactly zero gives code 0.0 and bit 0; the
    sample holding a NaN (the last one, inside a partial tile) is NaN in logits and codes with all bits 0; the sample holding
    +inf follows IEEE; and no other row differs from the run without the two: nothing leaks into tile neighbours or through
    the clamped rows of a partial tile."""
    E, n, B, pin, pset, kern = run
    assert tc.route(B, E, pin) == kern
    pinned(diag, pin)
    exact = tc.exact_case(E, n, B, pset)
    out = tc.run(exact, "gpu")
    tc.check_exact(exact, out)
    calm_case = tc.exact_case(E, n, B, pset, nonfinite=False)
    calm = tc.run(calm_case, "gpu")
    tc.check_exact(calm_case, calm)
    keep = [b for b in range(B) if b not in (exact["nan_row"], exact["inf_row"])]
    assert tc.same_bits({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in calm.items()})
    part = tc.run(exact, "gpu", ("packed",))
    assert tc.same_bits(part, {"packed": out["packed"]})


@POINT
def test_pins_reach_the_kernel_route_names(point, diag):
    """See the module text: a pin that falls through to a chain kernel equals the `simple` pin bit for bit; where route() says
    mfma (E >= 64, random data) the logits differ from the chain's in at least one bit, within twice the bound."""
    E, n, B = point
    case = tc.random_case(E, n, B, tc.SETS[list(tc.POINTS).index(point) % 4])
    _, tol = tc.reference(case)
    out = {}
    for pin in tc.PINS:
        pinned(diag, pin)
        out[pin] = tc.run(case, "gpu")
    for p, pin in enumerate(tc.PINS):
        kern = tc.route(B, E, pin)
        assert kern == tc.LETTER[tc.POINTS[point][p]]
        if kern != "mfma":
            assert tc.same_bits(out[pin], out["simple"]), pin
        else:
            assert tc.same_bits(out[pin], out["mfma"]), pin
            assert np.all(np.abs(out[pin]["logits"].astype(np.float64) - out["simple"]["logits"]) <= 2 * tol)
            if E >= 64:
                assert not np.array_equal(out[pin]["logits"], out["simple"]["logits"]), \
                    f"pin {pin}: bit-equal to the fmaf chain, so the matrix-core kernel did not run"


@pytest.mark.parametrize("pin", tc.KERNELS)
@pytest.mark.parametrize("nbits", [32, 96])
@pytest.mark.parametrize("E", [32, 416, 768])
def test_rows_do_not_depend_on_the_batch(E, nbits, pin, diag):
    """Rows [lo, hi) of a batch, run alone under the same pin, give the same bits.  (Unpinned this cannot hold across B = 32: a
    shorter batch goes to the chain kernels, another rounding.  A `valu16` pin hands short batches to `simple`, the same chain.)"""
    B = 65
    pinned(diag, pin)
    case = tc.random_case(E, nbits, B, tc.SETS[(E // 32 + nbits // 32) % 4])
    whole = tc.run(case, "gpu")
    for lo, hi in ((0, 1), (5, 37), (30, 37), (32, 65), (64, 65), (0, 64)):
        part = tc.run(tc.rows(case, lo, hi), "gpu")
        assert tc.same_bits(part, {k: v[lo:hi] for k, v in whole.items()}), (lo, hi)


@POINT
def test_kernels_and_host_twin_agree(point, diag):
    """Both meet the same bound against float64, so they lie within twice the bound of each other on random data; on the
    exact cases they are equal bit for bit."""
    E, n, B = point
    if E % 8:
        rc, _ = tc.call(tc.random_case(E, n, B, "plain"), "cpu")
        assert rc == tc.WV_EINVAL
        return
    pset = tc.SETS[(list(tc.POINTS).index(point) + 1) % 4]
    case, exact = tc.random_case(E, n, B, pset), tc.exact_case(E, n, B, pset)
    _, tol = tc.reference(case)
    twin, twin_exact = tc.run(case, "cpu"), tc.run(exact, "cpu")
    for pin in tc.KERNELS:
        pinned(diag, pin)
        out = tc.run(case, "gpu")
        assert np.all(np.abs(out["logits"].astype(np.float64) - twin["logits"]) <= 2 * tol), pin
        assert tc.same_bits(tc.run(exact, "gpu"), twin_exact), pin


def test_argument_refusals_return_before_any_launch(diag):
    pinned(diag, None)
    ok = tc.random_case(8, 96, 65, "bn")

    def refused(case, **kw):
        rc, bufs = tc.call(case, "gpu", **kw)
        fresh = tc.prefilled(kw.get("B", case["B"]), case["nbits"])
        assert all(np.array_equal(bufs[k], fresh[k]) for k in fresh), "outputs touched"
        return rc

    six = dict(ok, E=6, x=ok["x"][:, :6].copy(), w=ok["w"][:, :6].copy())
    assert refused(six) == tc.WV_EINVAL
    big = 12292                                                   # 4 E bytes: over 48 KB of LDS
    wide = dict(tc.random_case(8, 2, 1, "plain"), E=big, x=np.zeros((1, big), np.float32), w=np.zeros((2, big), np.float32))
    assert refused(wide) == tc.WV_EINVAL
    assert refused(dict(ok, nbits=0)) == tc.WV_EINVAL
    assert refused(dict(ok, bn_var=None)) == tc.WV_EINVAL
    assert refused(ok, B=0) == tc.WV_OK
    torch.cuda.synchronize()


class StubBackbone(torch.nn.Module):
    """[B, 3, H, W] -> {'x_norm_clstoken': [B, 768]}: 2 x 2 average pooling and one Linear, the width of dinov2_vitb14."""

    def __init__(self, seed=0):
        super().__init__()
        self.embed_dim = 768
        self.pool = torch.nn.AdaptiveAvgPool2d(2)
        self.proj = torch.nn.Linear(12, 768)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(768, 12, generator=g))
            self.proj.bias.copy_(0.1 * torch.randn(768, generator=g))

    def forward(self, x):
        return {"x_norm_clstoken": self.proj(self.pool(x).flatten(1))}


@pytest.mark.parametrize("nbits", [32, 96])
def test_vitb_width_baseline_model(nbits):
    """DINOHashBaseline at the width of its dinov2_vitb14 arms (E = 768, two load batches of the matrix-core kernel) with an odd
    number of 32-bit blocks: encode_packed (packed only) equals the packed forward codes, and the codes are the signs of the
    stock-PyTorch tail wherever its logit is further than the derived bound from zero."""
    from wvhash.engine import hamming as H
    from wvhash.models.single_band import DINOHashBaseline
    B = 40
    assert tc.route(B, 768, None) == "mfma"
    g = torch.Generator().manual_seed(nbits)
    model = DINOHashBaseline("dinov2_vitb14", embed_dim=768, binary_config={"nbits": nbits}, backbone=StubBackbone(1))
    bn = model.hash_head[1]
    with torch.no_grad():
        bn.running_mean.copy_(0.1 * torch.randn(nbits, generator=g)); bn.running_var.copy_(torch.rand(nbits, generator=g) * 1.5 + 0.5)
        bn.weight.copy_(torch.randn(nbits, generator=g)); bn.bias.copy_(0.1 * torch.randn(nbits, generator=g))
    model = model.cuda().eval()
    x = torch.rand(B, 3, 16, 16, generator=g).cuda()
    with torch.no_grad():
        codes = model(x)
        packed = model.encode_packed(x)
        feats = model.features(x)
        stock = model.hash_head(feats)
    assert tuple(codes.shape) == (B, nbits) and tuple(packed.shape) == (B, (nbits + 63) // 64)
    assert torch.equal(packed, H.pack_codes(codes))
    assert int((packed[:, -1] >> 32).abs().max()) == 0           # the half word above 32 / 96 bits
    case = {"E": 768, "nbits": nbits, "B": B, "kind": "random", "eps": bn.eps, "x": feats.cpu().numpy(),
            "w": model.hash_head[0].weight.detach().cpu().numpy(), "hb": None, "bn_w": bn.weight.detach().cpu().numpy(),
            "bn_b": bn.bias.detach().cpu().numpy(), "bn_mean": bn.running_mean.cpu().numpy(), "bn_var": bn.running_var.cpu().numpy()}
    ref, tol = tc.reference(case)
    far = torch.from_numpy(np.abs(stock.cpu().numpy().astype(np.float64)) > tol).cuda()
    assert float(far.float().mean()) > 0.99
    assert torch.equal(codes[far], torch.sign(stock)[far])
    assert np.array_equal(codes.cpu().numpy()[np.abs(ref) > tol], np.sign(ref)[np.abs(ref) > tol])
