"""Shared by the grouped-LayerNorm tests (host twin, kernel, module): the case list, the seeded inputs and the float64
reference -- torch.chunk and one F.layer_norm per group, in double.

Shapes are the smallest at which each path can break: E % 4 == 0 (four values per access) and not (one), E <= 512 (row in
registers) and above (loop path), half-used last accesses (E = 96, 100, 384), a single value per row (E = 1); every N / G
pairing of torch.chunk including N % G != 0 and N < G; row counts N * T that are no multiple of the four rows of a workgroup.
"""
import ctypes

import torch
import torch.nn.functional as F

from wvhash import _lib

DTYPES = (torch.float32, torch.bfloat16)
DT_CODE = {torch.float32: _lib.WV_DT_F32, torch.bfloat16: _lib.WV_DT_BF16}
KINDS = ("randn", "offset", "small", "const_row")
CONST = 2.5            # every partial sum of up to 1000 copies is exact in fp32 (and 2.5 is a bf16 value): mean == x exactly

ES = (384, 96, 100, 64, 1, 768, 30, 515, 1000)      # 768, 1000: loop path, 4 per access; 515: loop path, 1 per access; 30: 1 per access
NS = (1, 3, 4, 5, 6, 10)
TS = (1, 3, 7)
GS = (1, 2, 4)


def _cases():
    out = []
    for E in ES:                                     # every E with every input kind and both eps; 5 * 7 = 35 rows
        for k, kind in enumerate(KINDS):
            out.append(dict(N=5, T=7, E=E, G=4, kind=kind, eps=(1e-6, 1e-5)[k % 2]))
            out.append(dict(N=5, T=7, E=E, G=4, kind=kind, eps=(1e-5, 1e-6)[k % 2]))
    i = 0
    for N in NS:                                     # the group rule: every N with every G
        for G in GS:
            out.append(dict(N=N, T=3, E=96, G=G, kind=KINDS[i % 4], eps=1e-6))
            i += 1
    for T in TS:
        for N in (6, 10):
            out.append(dict(N=N, T=T, E=384, G=4, kind=KINDS[i % 4], eps=1e-6))
            i += 1
    return out


CASES = _cases()


def case_id(c):
    return f"N{c['N']}-T{c['T']}-E{c['E']}-G{c['G']}-{c['kind']}-eps{c['eps']:g}"


def const_row(c):
    """(n, t) of the constant row of a const_row case: in the last sequence, so that its group is the last one in use."""
    return c["N"] - 1, c["T"] // 2


def make_inputs(c, x_dtype=torch.float32, seed=0):
    """-> x [N, T, E] of x_dtype, gamma [G, E], beta [G, E] (fp32, different per group so that a wrong group shows)."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * c["N"] + 13 * c["T"] + 17 * c["E"] + 19 * c["G"])
    N, T, E, G = c["N"], c["T"], c["E"], c["G"]
    x = torch.randn(N, T, E, generator=g)
    if c["kind"] == "offset":
        x = 3 * x + 5
    elif c["kind"] == "small":
        x = 0.02 * x
    elif c["kind"] == "const_row":
        n, t = const_row(c)
        x[n, t] = CONST
    gamma = 1.0 + 0.5 * torch.randn(G, E, generator=g) + torch.arange(G).float()[:, None]
    beta = 0.3 * torch.randn(G, E, generator=g) - torch.arange(G).float()[:, None]
    return x.to(x_dtype).contiguous(), gamma.contiguous(), beta.contiguous()


def chunk_norm_cat(x, gamma, beta, eps, G):
    """The reference module's forward on plain tensors, in x's dtype family: fp32 in -> fp32, float64 in -> float64."""
    E = x.shape[-1]
    chunks = x.chunk(G, dim=0)
    return torch.cat([F.layer_norm(ch, (E,), gamma[i].to(x.dtype), beta[i].to(x.dtype), eps) for i, ch in enumerate(chunks)], dim=0)


def reference_f64(x, gamma, beta, eps, G):
    return chunk_norm_cat(x.double(), gamma.double(), beta.double(), eps, G)


def run_twin(x, gamma, beta, eps, G, out_dtype):
    """wv_group_layernorm_cpu through ctypes on host tensors."""
    N, T, E = x.shape
    out = torch.empty(x.shape, dtype=out_dtype)
    rc = _lib.load().wv_group_layernorm_cpu(_lib.ptr(x), DT_CODE[x.dtype], _lib.ptr(out), DT_CODE[out_dtype], N, T, E, G,
                                            _lib.ptr(gamma), _lib.ptr(beta), ctypes.c_float(eps))
    _lib.check(rc, "wv_group_layernorm_cpu")
    return out


def bits(t):
    """The tensor's raw bits as integers, for bit-for-bit comparisons."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
