"""The grouped LayerNorm kernel against the stock chunk / norm / cat module, in ONE run, at the token tensors of the c1 batch
(B = 2048 images -> 8192 sequences, 384 wide): [8192, 267, 384] (10 prompts) and [8192, 257, 384] (no prompts).

    python tools/bench_group_layernorm.py [--out profiles/group_layernorm.json] [--sequences 8192] [--rounds 7] [--calls 4]

Per shape and dtype pair (fp32 -> fp32, fp32 -> bf16), timed with HIP events around single calls after a warm-up that also
ramps the clock, variants alternating inside every round, median over rounds x calls calls (>= 20):
  kernel_ms   wv_group_layernorm: one launch, x read once, out written once
  stock_ms    the reference module's forward: x.chunk(4, 0), four nn.LayerNorm, torch.cat; for the bf16 pair followed by
              .to(bfloat16), which is what the next autocast Linear does to the stock fp32 output
  max_abs_diff  kernel against stock on the whole tensor (checked before anything is timed)
Bytes: the ALGORITHMIC bytes of the kernel (input once, output once, the [4, 384] parameters ignored) and, for the stock
path, what its steps move by the same counting (norms: read + write, cat: read + write, cast: read + write); GB/s of the
kernel over its bytes, and that as a fraction of 8 TB/s (HBM peak).  Prints one JSON row.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn as nn

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash.models import MultiDomainLayerNorm, group_layernorm  # noqa: E402

E = 384
TOKENS = (267, 257)
PAIRS = ((torch.float32, torch.float32), (torch.float32, torch.bfloat16))
HBM_PEAK = 8e12


def one_call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def size(dtype):
    return 4 if dtype == torch.float32 else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sequences", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group_layernorm: needs the GPU (a rate measured elsewhere says nothing about it)")
    N = args.sequences
    g = torch.Generator().manual_seed(1)
    module = MultiDomainLayerNorm(nn.LayerNorm(E, eps=1e-6), num_domains=4)
    with torch.no_grad():
        for norm in module.norms:
            norm.weight.copy_(1.0 + 0.1 * torch.randn(E, generator=g))
            norm.bias.copy_(0.1 * torch.randn(E, generator=g))
    module = module.cuda()
    gamma = torch.stack([n.weight.detach() for n in module.norms]).contiguous()
    beta = torch.stack([n.bias.detach() for n in module.norms]).contiguous()

    def stock(x):
        return torch.cat([module.norms[i](ch) for i, ch in enumerate(x.chunk(4, dim=0))], dim=0)

    configs = []
    for T in TOKENS:
        x = torch.randn(N, T, E, device="cuda", generator=torch.Generator("cuda").manual_seed(T))
        values = N * T * E
        for x_dtype, out_dtype in PAIRS:
            with torch.no_grad():
                if out_dtype == torch.float32:
                    stock_fn = lambda: stock(x)                                     # noqa: E731
                else:
                    stock_fn = lambda: stock(x).to(torch.bfloat16)                  # noqa: E731
                kernel_fn = lambda: group_layernorm(x, gamma, beta, 1e-6, out_dtype=out_dtype)      # noqa: E731
                diff = float((kernel_fn().float() - stock_fn().float()).abs().max())
                variants = {"kernel": kernel_fn, "stock": stock_fn}
                for _ in range(10):                                                 # warm-up: code objects, allocator, clocks
                    for fn in variants.values():
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in variants}
                for _ in range(args.rounds):                                        # alternating
                    for k, fn in variants.items():
                        ms[k] += [one_call_ms(fn) for _ in range(args.calls)]
            med = {k: statistics.median(v) for k, v in ms.items()}
            kernel_bytes = values * (size(x_dtype) + size(out_dtype))
            stock_bytes = values * 4 * 4 + (values * (4 + 2) if out_dtype == torch.bfloat16 else 0)
            gbs = kernel_bytes / (med["kernel"] * 1e-3) / 1e9
            configs.append({"shape": [N, T, E], "x": "f32", "out": "f32" if out_dtype == torch.float32 else "bf16",
                            "max_abs_diff": diff, "calls_per_variant": args.rounds * args.calls,
                            "kernel_ms": round(med["kernel"], 4), "kernel_ms_min": round(min(ms["kernel"]), 4),
                            "stock_ms": round(med["stock"], 4), "stock_ms_min": round(min(ms["stock"]), 4),
                            "speedup": round(med["stock"] / med["kernel"], 3), "kernel_faster": bool(med["kernel"] < med["stock"]),
                            "kernel_bytes": kernel_bytes, "stock_bytes": stock_bytes, "kernel_GBps": round(gbs, 1),
                            "stock_GBps": round(stock_bytes / (med["stock"] * 1e-3) / 1e9, 1),
                            "kernel_hbm_fraction": round(gbs * 1e9 / HBM_PEAK, 4)})
        del x
        torch.cuda.empty_cache()
    row = {"what": "wv_group_layernorm against chunk / 4 x nn.LayerNorm / cat (4 domains), same session, alternating",
           "device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM_PEAK, "configs": configs}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
