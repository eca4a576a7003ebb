#!/usr/bin/env python3
"""Regenerates tests/golden/head_bf16_golden.npz.  Run in the BUILD container only (needs /root/reference):
    python tests/golden/make_golden_head_bf16.py

What the file pins: how far the REFERENCE's own fusion-head modules move when they run in bf16.  For the seven
configurations of make_golden.py::HEAD_CASES (same seeds, weights from wvhash.synth.head_state, B = 16), with the band
features rounded to bf16 first so that every path sees the same inputs:
  <case>/out32  the reference module's plain fp32 eval output
  <case>/out16  the same module under torch.autocast("cpu", dtype=torch.bfloat16) fed bf16 features (uint16 bit patterns)
  <case>/gap    [max, rms] of out16 - out32
  <case>/meta, qscale, sha as in head_golden.npz
The gap is the yardstick of the bf16 matrix-core head (tests/test_host_head_bf16.py, tests/test_gpu_head_bf16.py): a bf16
implementation must be no further from out32 than the reference's own bf16 run is.  The script also prints where a torch
emulation of the library's contract (operands of the five weight products rounded to bf16, everything else fp32) sits
relative to that gap.  Fixtures are data only: inputs are regenerated from seeds, outputs are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (sets sys.path for oracle / wvhash)
from oracle import head_torch  # noqa: E402
from wvhash import synth  # noqa: E402

B = 16


def bf16_features(batch, E, seed):
    return [f.bfloat16().float() for f in synth.band_features(batch, E, seed)]


def contract_emulation(feats, sd, heads, pool, normalize, round_outputs=False):
    """Contract section 1 in torch (fp64 accumulation stands in for fp32: the difference is 1e-7): operands of the five
    weight products rounded to bf16; round_outputs also rounds every product's output (the other allowed design)."""
    r = lambda t: t.bfloat16().double()
    o = (lambda t: r(t)) if round_outputs else (lambda t: t)
    g = lambda k: sd[k].double()
    kv = torch.stack([f.double() for f in feats], dim=1)
    Bn, S, E = kv.shape
    q = head_torch.effective_queries(sd, normalize).double().expand(Bn, -1, -1)
    Nq, hd = q.shape[1], E // heads
    w_in, b_in = g("attn.in_proj_weight"), g("attn.in_proj_bias")
    Q = q @ w_in[:E].t() + b_in[:E]
    KV = o(r(kv) @ r(w_in[E:]).t()) + b_in[E:]
    K, V = KV[..., :E], KV[..., E:]
    sp = lambda t, n: t.reshape(Bn, n, heads, hd).transpose(1, 2)
    P = torch.softmax(sp(Q, Nq) @ sp(K, S).transpose(-1, -2) / hd ** 0.5, dim=-1)
    ctx = (P @ sp(V, S)).transpose(1, 2).reshape(Bn, Nq, E)
    ln = torch.nn.functional.layer_norm
    x = ln(q + o(r(ctx) @ r(g("attn.out_proj.weight")).t()) + g("attn.out_proj.bias"), (E,), g("norm1.weight"), g("norm1.bias"))
    h = torch.nn.functional.gelu(o(r(x) @ r(g("mlp.0.weight")).t()) + g("mlp.0.bias"))
    x = x + o(r(h) @ r(g("mlp.2.weight")).t()) + g("mlp.2.bias")
    x = x.mean(dim=1) if pool == "mean" else x.reshape(Bn, -1)
    x = o(r(x) @ r(g("out_proj.weight")).t()) + g("out_proj.bias")
    return ln(x, (E,), g("norm2.weight"), g("norm2.bias")).float()


def main():
    mda = mg.load_reference_heads()
    out = {}
    for name, ftype, E, heads, nq, extra, _, seed in mg.HEAD_CASES:
        cfg = {"type": ftype, "output_dim": E, "num_heads": heads, "dropout": 0.1, "num_queries": nq,
               "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
        cfg.update(extra)
        head = mda.get_fusion_head(cfg, [E] * 4).eval()
        pool = "mean" if extra.get("query_pool") == "mean" else "concat"
        qs = extra.get("query_scale_init")
        sd = synth.head_state(E, nq, pool, seed, query_scale=qs)
        head.load_state_dict(sd, strict=True)
        feats = bf16_features(B, E, seed + 1000)
        with torch.no_grad():
            y32 = head([f.clone() for f in feats])
            with torch.autocast("cpu", dtype=torch.bfloat16):
                y16 = head([f.bfloat16() for f in feats])
        assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
        d = y16.float() - y32
        gap = np.array([float(d.abs().max()), float(d.pow(2).mean().sqrt())])
        out[f"{name}/out32"] = y32.numpy()
        out[f"{name}/out16"] = y16.view(torch.int16).numpy().view(np.uint16)
        out[f"{name}/gap"] = gap
        out[f"{name}/meta"] = np.array([E, heads, nq, B, seed, 1 if pool == "mean" else 0,
                                        1 if ftype.endswith("decoupled") else 0], dtype=np.int64)
        out[f"{name}/qscale"] = np.array([qs if qs is not None else 0.0], dtype=np.float32)
        out[f"{name}/sha"] = np.frombuffer(bytes.fromhex(synth.state_sha(sd)), dtype=np.uint8)
        line = f"head_bf16 {name}: gap max {gap[0]:.4f} rms {gap[1]:.5f};"
        for label, ro in (("operands only", False), ("outputs rounded too", True)):
            e = contract_emulation(feats, sd, heads, pool, ftype.endswith("decoupled"), ro) - y32
            line += f"  {label}: rms {float(e.pow(2).mean().sqrt()) / gap[1]:.2f} x, max {float(e.abs().max()) / gap[0]:.2f} x;"
        print(line)
    path = os.path.join(HERE, "head_bf16_golden.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(1)
    main()
