"""Per-domain LayerNorm of the prompt-tuned shared backbone: class name, parameters and state_dict keys of the reference's
MultiDomainLayerNorm / inject_domain_specific_layernorms (main/models/multi_dino_attention.py:902-940).

The reference's forward is ``x.chunk(num_domains, 0)`` -> one ``nn.LayerNorm`` per chunk -> ``torch.cat``: every value is read
and written twice.  Without gradients the module runs the library's one-pass kernel instead (``wv_group_layernorm``; host
tensors take its host twin when ``host_twin = True``); with gradients, and for everything the kernel does not cover, it
runs the reference's three steps as stock PyTorch.  A missing library is an error, never a silent stock run.
"""
import torch
import torch.nn as nn

from .. import _lib
from ._prepared import PreparedCache, param_key

_DTYPES = {torch.float32: _lib.WV_DT_F32, torch.bfloat16: _lib.WV_DT_BF16}


def group_layernorm(x, gamma, beta, eps, out_dtype=None, host_twin=False):
    """x [N, T, E] (contiguous fp32 / bf16) -> LayerNorm over E with gamma[g], beta[g] ([G, E] fp32) for the sequences of
    ``x.chunk(G, 0)[g]``, as ``out_dtype`` (fp32 / bf16; default: x's).  GPU tensors: the HIP kernel on the current stream;
    host tensors: only with ``host_twin=True``, the library's host twin (bit-identical to the kernel)."""
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if x.dim() != 3 or not x.is_contiguous() or x.dtype not in _DTYPES or out_dtype not in _DTYPES:
        raise ValueError(f"group_layernorm: x must be a contiguous fp32 / bf16 [N, T, E] tensor and out_dtype fp32 / bf16, got "
                         f"{tuple(x.shape)} {x.dtype} -> {out_dtype}")
    N, T, E = x.shape
    G = gamma.shape[0]
    for name, p in (("gamma", gamma), ("beta", beta)):
        if p.dtype != torch.float32 or tuple(p.shape) != (G, E) or not p.is_contiguous() or p.device != x.device:
            raise ValueError(f"group_layernorm: {name} must be a contiguous fp32 [{G}, {E}] tensor on {x.device}")
    host = not x.is_cuda
    if host and not host_twin:
        raise _lib.WvhashUnavailable("group_layernorm: host tensor without host_twin=True (there is no silent CPU path)")
    lib = _lib.load() if host else _lib.require_gpu()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    args = (_lib.ptr(x), _DTYPES[x.dtype], _lib.ptr(out), _DTYPES[out_dtype], N, T, E, G, _lib.ptr(gamma), _lib.ptr(beta), float(eps))
    if host:
        _lib.check(lib.wv_group_layernorm_cpu(*args), "wv_group_layernorm_cpu")
    else:
        with torch.cuda.device(x.device):
            _lib.check(lib.wv_group_layernorm(*args, _lib.stream_ptr()), "wv_group_layernorm")
    return out


class MultiDomainLayerNorm(nn.Module):
    """``emit_dtype``: None (what stock PyTorch gives: fp32 under autocast, else the input's dtype), torch.bfloat16, or
    "auto" = bf16 exactly under bf16 autocast on the GPU -- for a norm whose only reader is an autocast Linear, which rounds
    the fp32 result to bf16 anyway: one rounding either way, the same bits.  Library path only; the stock path ignores it.
    ``kernel_calls`` / ``stock_calls`` count the forwards of each path."""

    emit_dtype = None
    host_twin = False

    def __init__(self, original_norm, num_domains=4):
        super().__init__()
        self.num_domains = num_domains
        self.norms = nn.ModuleList([
            nn.LayerNorm(original_norm.normalized_shape, eps=original_norm.eps,
                         elementwise_affine=original_norm.elementwise_affine)
            for _ in range(num_domains)])
        if original_norm.elementwise_affine:
            with torch.no_grad():
                for norm in self.norms:
                    norm.weight.copy_(original_norm.weight)
                    norm.bias.copy_(original_norm.bias)
        self.kernel_calls = 0
        self.stock_calls = 0
        self._prepared = PreparedCache()    # slot "affine": (gamma [G, E], beta [G, E]), rebuilt when a parameter changes or moves

    def _affine(self, device):
        def build():
            with torch.no_grad():
                gamma = torch.stack([norm.weight.detach().float() for norm in self.norms]).contiguous()
                beta = torch.stack([norm.bias.detach().float() for norm in self.norms]).contiguous()
            return gamma, beta
        params = [p for norm in self.norms for p in (norm.weight, norm.bias)]
        return self._prepared.get("affine", device, param_key(*params), build)

    def _library_path(self, x):
        first = self.norms[0]
        if first.weight is None or first.bias is None or len(first.normalized_shape) != 1:
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.norms.parameters())):
            return False
        if x.dim() < 2 or x.dtype not in _DTYPES or not x.is_contiguous() or x.shape[-1] != first.normalized_shape[0]:
            return False
        if any(p.device != x.device for p in self.norms.parameters()):
            return False
        if x.is_cuda:
            return True
        return bool(self.host_twin) and x.device.type == "cpu" and not torch.is_autocast_enabled("cpu")

    def _out_dtype(self, x):
        autocast = x.is_cuda and torch.is_autocast_enabled("cuda")
        if self.emit_dtype == "auto":
            if autocast and torch.get_autocast_dtype("cuda") == torch.bfloat16:
                return torch.bfloat16
        elif self.emit_dtype is not None:
            return self.emit_dtype
        return torch.float32 if autocast else x.dtype       # autocast runs layer_norm in fp32

    def forward(self, x):
        if not self._library_path(x):
            self.stock_calls += 1
            chunks = x.chunk(self.num_domains, dim=0)
            return torch.cat([self.norms[i](chunk) for i, chunk in enumerate(chunks)], dim=0)
        self.kernel_calls += 1
        gamma, beta = self._affine(x.device)
        x3 = x.reshape(x.shape[0], -1, x.shape[-1])          # a view: x is contiguous
        out = group_layernorm(x3, gamma, beta, self.norms[0].eps, out_dtype=self._out_dtype(x), host_twin=not x.is_cuda)
        return out.view(x.shape)


def inject_domain_specific_layernorms(model, num_domains=4):
    """Replaces the ViT's shared LayerNorms with per-domain MultiDomainLayerNorms."""
    for blk in model.blocks:
        blk.norm1 = MultiDomainLayerNorm(blk.norm1, num_domains)
        blk.norm2 = MultiDomainLayerNorm(blk.norm2, num_domains)
    if hasattr(model, 'norm') and model.norm is not None:
        model.norm = MultiDomainLayerNorm(model.norm, num_domains)
    return model
