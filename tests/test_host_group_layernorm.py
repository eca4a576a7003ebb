"""The host twin of the grouped LayerNorm (wv_group_layernorm_cpu; no GPU) against a float64 reference, and the module's
library path on the host (host_twin = True) against the reference module's chunk / norm / cat.

Accuracy bound (fp32 out): the twin's largest error against float64 may be at most 4 x the largest error of stock
F.layer_norm in fp32 on the same input -- both errors are computed here.  The margin covers the different order of the
sums (64 lane-strided partial sums and a butterfly against ATen's vectorised row sums); nothing else differs."""
import ctypes

import pytest
import torch
import torch.nn as nn

import group_layernorm_cases as GC
from wvhash import _lib
from wvhash.models import MultiDomainLayerNorm, group_layernorm, inject_domain_specific_layernorms

MARGIN = 4.0


@pytest.mark.parametrize("c", GC.CASES, ids=GC.case_id)
def test_twin_against_float64(c):
    for x_dtype in GC.DTYPES:
        x, gamma, beta = GC.make_inputs(c, x_dtype)
        ref = GC.reference_f64(x, gamma, beta, c["eps"], c["G"])
        stock = GC.chunk_norm_cat(x.float(), gamma, beta, c["eps"], c["G"])
        got = GC.run_twin(x, gamma, beta, c["eps"], c["G"], torch.float32)
        err_twin = float((got.double() - ref).abs().max())
        err_stock = float((stock.double() - ref).abs().max())
        print(f"{GC.case_id(c)} {x_dtype}: twin {err_twin:.3e} stock {err_stock:.3e} ratio {err_twin / max(err_stock, 1e-30):.2f}")
        assert err_twin <= MARGIN * err_stock, (x_dtype, err_twin, err_stock)
        # bf16 out = the fp32 output rounded once, to nearest even
        got16 = GC.run_twin(x, gamma, beta, c["eps"], c["G"], torch.bfloat16)
        assert torch.equal(GC.bits(got16), GC.bits(got.to(torch.bfloat16))), x_dtype
        if c["kind"] == "const_row":
            n, t = GC.const_row(c)
            group = n // -(-c["N"] // c["G"])
            assert torch.equal(got[n, t], beta[group])
            assert torch.equal(got16[n, t], beta[group].to(torch.bfloat16))


@pytest.mark.parametrize("N", GC.NS)
@pytest.mark.parametrize("G", GC.GS)
def test_group_rule_matches_the_reference_module(N, G):
    """Per-domain parameters far apart: a sequence normalised with another group's would be off by about 1."""
    c = dict(N=N, T=3, E=96, G=G, kind="randn", eps=1e-6)
    x, gamma, beta = GC.make_inputs(c)
    module = MultiDomainLayerNorm(nn.LayerNorm(96, eps=1e-6), num_domains=G)
    with torch.no_grad():
        for d, norm in enumerate(module.norms):
            norm.weight.copy_(gamma[d])
            norm.bias.copy_(beta[d])
    with torch.no_grad():
        want = module(x)                                         # host, no host_twin: the reference's three steps
        assert (module.stock_calls, module.kernel_calls) == (1, 0)
        module.host_twin = True
        got = module(x)
        assert (module.stock_calls, module.kernel_calls) == (1, 1)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert float((got - want).abs().max()) <= 1e-5
    assert torch.equal(got, GC.run_twin(x, gamma, beta, 1e-6, G, torch.float32))


def test_module_keeps_the_reference_keys_and_takes_the_stock_path_with_gradients():
    module = MultiDomainLayerNorm(nn.LayerNorm(64, eps=1e-5), num_domains=4)
    assert sorted(module.state_dict()) == sorted(f"norms.{d}.{p}" for d in range(4) for p in ("weight", "bias"))
    assert module.emit_dtype is None
    module.host_twin = True
    x = torch.randn(8, 3, 64)
    module(x)                                                    # parameters require grad, grad mode on
    assert (module.stock_calls, module.kernel_calls) == (1, 0)
    with torch.no_grad():
        y = module(x)
        assert (module.stock_calls, module.kernel_calls) == (1, 1)
        module(x.half())                                         # a dtype the kernel does not cover
        module(x.transpose(0, 1))                                # not contiguous
        assert (module.stock_calls, module.kernel_calls) == (3, 1)
        with torch.no_grad():                                    # a changed parameter is seen by the next call
            module.norms[1].bias.add_(1.0)
        y2 = module(x)
        assert float((y2[2:4] - y[2:4] - 1.0).abs().max()) <= 1e-6 and torch.equal(y2[:2], y[:2])
    plain = MultiDomainLayerNorm(nn.LayerNorm(64, elementwise_affine=False))
    plain.host_twin = True
    with torch.no_grad():
        plain(x)
    assert (plain.stock_calls, plain.kernel_calls) == (1, 0)     # not affine: stock


def test_inject_replaces_every_layernorm():
    from wvhash.models.vit import tiny_vit
    vit = inject_domain_specific_layernorms(tiny_vit(img_size=28), num_domains=4)
    norms = [blk.norm1 for blk in vit.blocks] + [blk.norm2 for blk in vit.blocks] + [vit.norm]
    assert all(isinstance(m, MultiDomainLayerNorm) and m.emit_dtype is None and m.norms[0].eps == 1e-6 for m in norms)
    assert "blocks.1.norm2.norms.3.bias" in vit.state_dict() and "norm.norms.0.weight" in vit.state_dict()


def test_argument_errors_and_zero_rows():
    lib = _lib.load()
    F32, BF16 = _lib.WV_DT_F32, _lib.WV_DT_BF16
    x = torch.randn(2, 3, 8)
    out = torch.full((2, 3, 8), 7.0)
    gamma, beta = torch.ones(2, 8), torch.zeros(2, 8)
    eps = ctypes.c_float(1e-5)

    def call(xp=x, xd=F32, op=out, od=F32, N=2, T=3, E=8, G=2, gp=gamma, bp=beta):
        return lib.wv_group_layernorm_cpu(_lib.ptr(xp), xd, _lib.ptr(op), od, N, T, E, G, _lib.ptr(gp), _lib.ptr(bp), eps)

    def refused(rc, word):
        assert rc == -22
        msg = lib.wv_last_error().decode()
        assert word in msg, msg

    assert lib.wv_group_layernorm_check(F32, BF16, 2, 3, 8, 2) == 0
    refused(lib.wv_group_layernorm_check(_lib.WV_DT_U8, F32, 2, 3, 8, 2), "x_dtype")
    refused(lib.wv_group_layernorm_check(F32, 7, 2, 3, 8, 2), "out_dtype")
    refused(lib.wv_group_layernorm_check(F32, F32, 2, 3, 0, 2), "E =")
    refused(lib.wv_group_layernorm_check(F32, F32, 2, 3, 8, 0), "G =")
    refused(lib.wv_group_layernorm_check(F32, F32, -1, 3, 8, 2), "N =")
    refused(lib.wv_group_layernorm_check(F32, F32, 2, -3, 8, 2), "T =")
    assert lib.wv_group_layernorm_check(F32, F32, 1 << 40, 1 << 40, 8, 2) == _lib.WV_ENOTSUP
    refused(call(xd=_lib.WV_DT_U8), "x_dtype")
    refused(call(od=9), "out_dtype")
    refused(call(E=0), "E =")
    refused(call(G=0), "G =")
    refused(call(xp=None), "x is NULL")
    refused(call(op=None), "out is NULL")
    refused(call(gp=None), "gamma is NULL")
    refused(call(bp=None), "beta is NULL")
    refused(call(op=x), "out == x")
    assert torch.equal(out, torch.full((2, 3, 8), 7.0))          # nothing was written by a refused call
    for N, T in ((0, 3), (2, 0)):                                 # zero rows: OK, nothing touched, pointers not looked at
        assert call(N=N, T=T) == 0 and call(N=N, T=T, xp=None, op=None, gp=None, bp=None) == 0
    assert torch.equal(out, torch.full((2, 3, 8), 7.0))
    with pytest.raises(ValueError, match="E ="):
        _lib.check(call(E=-4), "wv_group_layernorm_cpu")
    with pytest.raises(_lib.WvhashUnavailable):
        group_layernorm(x, gamma, beta, 1e-5)                     # a host tensor without host_twin: never a silent path
    assert call() == 0 and not torch.equal(out, torch.full((2, 3, 8), 7.0))
