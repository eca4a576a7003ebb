"""The grouped LayerNorm kernel (wv_group_layernorm) on the GPU: equal to its host twin bit for bit on every case and dtype
pairing; the module's library path against the stock chunk / norm / cat module under the twin's accuracy rule; bf16 emission
under autocast; the stock path, with the reference's gradients, whenever a gradient is needed."""
import pytest
import torch
import torch.nn as nn

import group_layernorm_cases as GC
from wvhash.models import MultiDomainLayerNorm, group_layernorm

pytestmark = pytest.mark.gpu

MARGIN = 4.0


def module_for(gamma, beta, eps):
    G, E = gamma.shape
    module = MultiDomainLayerNorm(nn.LayerNorm(E, eps=eps), num_domains=G)
    with torch.no_grad():
        for d, norm in enumerate(module.norms):
            norm.weight.copy_(gamma[d])
            norm.bias.copy_(beta[d])
    return module.cuda()


def stock_forward(module, x):
    """The reference module's forward on the module's own LayerNorms."""
    return torch.cat([module.norms[i](ch) for i, ch in enumerate(x.chunk(module.num_domains, dim=0))], dim=0)


@pytest.mark.parametrize("c", GC.CASES, ids=GC.case_id)
def test_kernel_equals_twin_bit_for_bit(c):
    for x_dtype in GC.DTYPES:
        x, gamma, beta = GC.make_inputs(c, x_dtype)
        xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()
        for out_dtype in GC.DTYPES:
            want = GC.run_twin(x, gamma, beta, c["eps"], c["G"], out_dtype)
            got = group_layernorm(xg, gg, bg, c["eps"], out_dtype=out_dtype)
            assert got.dtype == out_dtype and got.shape == x.shape
            assert torch.equal(GC.bits(got.cpu()), GC.bits(want)), (x_dtype, out_dtype)


def test_unaligned_pointers_move_the_same_values():
    """A view that starts 4 bytes into its storage: the kernel's single-value accesses, the same sums, the same bits."""
    c = dict(N=5, T=7, E=384, G=4, kind="randn", eps=1e-6)
    x, gamma, beta = GC.make_inputs(c)
    flat = torch.empty(x.numel() + 1, device="cuda")
    shifted = flat[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = group_layernorm(shifted, gamma.cuda(), beta.cuda(), 1e-6)
    assert torch.equal(got.cpu(), GC.run_twin(x, gamma, beta, 1e-6, 4, torch.float32))


@pytest.mark.parametrize("c", [c for c in GC.CASES if c["E"] in (384, 100, 515) and c["eps"] == 1e-6], ids=GC.case_id)
def test_module_against_the_stock_module(c):
    x, gamma, beta = GC.make_inputs(c)
    module = module_for(gamma, beta, c["eps"])
    ref = GC.reference_f64(x, gamma, beta, c["eps"], c["G"])
    with torch.no_grad():
        got = module(x.cuda())
        stock = stock_forward(module, x.cuda())
    assert (module.kernel_calls, module.stock_calls) == (1, 0)
    assert got.dtype == stock.dtype and got.shape == stock.shape
    err_kernel = float((got.cpu().double() - ref).abs().max())
    err_stock = float((stock.cpu().double() - ref).abs().max())
    print(f"{GC.case_id(c)}: kernel {err_kernel:.3e} stock {err_stock:.3e}")
    assert err_kernel <= MARGIN * err_stock


def test_output_dtype_follows_stock_pytorch_and_emit_dtype():
    c = dict(N=6, T=7, E=384, G=4, kind="offset", eps=1e-6)
    x, gamma, beta = GC.make_inputs(c)
    module = module_for(gamma, beta, 1e-6)
    xg = x.cuda()
    with torch.no_grad():
        assert module(xg).dtype == torch.float32
        assert module(xg.bfloat16()).dtype == torch.bfloat16     # (stock refuses bf16 input with fp32 parameters outside autocast)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            stock = stock_forward(module, xg)
            plain = module(xg)
            assert plain.dtype == stock.dtype == torch.float32           # autocast runs layer_norm in fp32
            assert module(xg.bfloat16()).dtype == stock_forward(module, xg.bfloat16()).dtype
            module.emit_dtype = "auto"
            emitted = module(xg)
        assert emitted.dtype == torch.bfloat16
        assert torch.equal(GC.bits(emitted.cpu()), GC.bits(plain.to(torch.bfloat16).cpu()))      # one rounding of the fp32 result
        # ... which is what the next autocast Linear makes of the stock output, within the 4x rule on the fp32 values
        ref = GC.reference_f64(x, gamma, beta, 1e-6, 4)
        assert float((plain.cpu().double() - ref).abs().max()) <= MARGIN * float((stock.cpu().double() - ref).abs().max())
        assert module(xg).dtype == torch.float32                         # "auto" outside autocast: the stock dtype
        with torch.autocast("cuda", dtype=torch.float16):
            assert module(xg).dtype == torch.float32                     # "auto" emits bf16 under bf16 autocast only
        module.emit_dtype = torch.bfloat16
        assert module(xg).dtype == torch.bfloat16
    assert module.stock_calls == 0


def test_gradients_take_the_stock_path_and_equal_the_reference():
    c = dict(N=6, T=3, E=96, G=4, kind="randn", eps=1e-5)
    x, gamma, beta = GC.make_inputs(c)
    module = module_for(gamma, beta, 1e-5)
    xg = x.cuda().requires_grad_(True)
    out = module(xg)
    assert (module.kernel_calls, module.stock_calls) == (0, 1)
    weight = torch.linspace(-1, 1, out.numel(), device="cuda").view(out.shape)
    (out * weight).sum().backward()
    ref_module = module_for(gamma, beta, 1e-5)
    xr = x.cuda().requires_grad_(True)
    (stock_forward(ref_module, xr) * weight).sum().backward()
    assert torch.equal(xg.grad, xr.grad)
    for d, (mine, theirs) in enumerate(zip(module.norms, ref_module.norms)):
        if d == 3:                                                       # 6 sequences make 3 chunks: the fourth norm is unused
            assert mine.weight.grad is None and theirs.weight.grad is None
            continue
        assert torch.equal(mine.weight.grad, theirs.weight.grad) and torch.equal(mine.bias.grad, theirs.bias.grad)
    for p in module.parameters():
        p.requires_grad_(False)
    module(x.cuda())                                                     # grad mode on, nothing requires grad: the kernel
    assert (module.kernel_calls, module.stock_calls) == (1, 1)
