"""The pairwise hashing losses in ONE run: loss + backward to the embeddings through the fused path (wv_pair_loss behind
wvhash.losses' autograd Function) against the plain PyTorch path of the SAME module on the same GPU, for SCHLoss(alpha = 1,
beta = 1, apply_tanh) and HashNetAdapter, at B = 64, 96, 128, 1024 rows of D = 64 logits, 38 classes at p = 0.08.

    python tools/bench_pair_loss.py [--out profiles/pair_loss.json] [--rounds 6] [--calls 5]

One call = module(embeddings, labels) then .backward() into embeddings.grad: what train_step pays per step for the loss
(label packing and the 0/1 label check with its synchronise included on the fused side).  Per batch size, after a warm-up of
both variants, variants alternating inside every round, median [min, max] over rounds x calls (>= 20) single calls, HIP
events around the call.  The two paths' numbers are compared first (value relative, gradient norm-wise).  Times of calls
this short are launch and host-dispatch times as much as kernel times: they are what a caller waits for on the stream, not
a kernel's share of any peak.  Prints one JSON row.
"""
import argparse
import json
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import losses as L  # noqa: E402

BATCHES, D, CLASSES, P_TAG = (64, 96, 128, 1024), 64, 38, 0.08


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def modules():
    return {"sch": lambda: L.SCHLoss(n_bits=D, alpha=1, beta=1, apply_tanh=True), "hashnet": lambda: L.HashNetAdapter(embedding_size=D)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_loss: needs the GPU (a time measured elsewhere says nothing about it)")
    rows = []
    for kind, make in modules().items():
        for B in BATCHES:
            g = torch.Generator().manual_seed(B)
            emb = (1.5 * torch.randn(B, D, generator=g)).cuda().requires_grad_(True)
            lab = (torch.rand(B, CLASSES, generator=g) < P_TAG).float().cuda()
            fused, plain = make(), make()
            fused.fused, plain.fused = True, False

            def step(module):
                emb.grad = None
                val = module(emb, lab)
                val.backward()
                return val.detach(), emb.grad

            variants = {"fused": lambda: step(fused), "plain": lambda: step(plain)}
            (fv, fg), (pv, pg) = variants["fused"](), variants["plain"]()
            dv = abs(float(fv) - float(pv)) / abs(float(pv))
            dg = float((fg - pg).abs().max() / pg.abs().max())
            for _ in range(5):                                                   # warm-up: code objects, allocator, clocks
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            ms = {v: [] for v in variants}
            for _ in range(args.rounds):                                         # alternating
                for v, fn in variants.items():
                    ms[v] += [event_ms(fn) for _ in range(args.calls)]
            med = {v: statistics.median(t) for v, t in ms.items()}
            rows.append({"loss": kind, "B": B, "D": D, "value_rel_diff": dv, "grad_normwise_diff": dg,
                         "calls_per_variant": args.rounds * args.calls, "fused": spread(ms["fused"]), "plain": spread(ms["plain"]),
                         "plain_over_fused": round(med["plain"] / med["fused"], 3),
                         "fused_faster_than_plain": bool(med["fused"] < med["plain"])})
    row = {"what": "loss + backward to the embeddings: wv_pair_loss behind the autograd Function (fused) against the plain "
                   "PyTorch path of the same module; SCHLoss(alpha=1, beta=1, apply_tanh=True), HashNetAdapter at scale 1",
           "device": torch.cuda.get_device_name(0), "classes": CLASSES, "p_tag": P_TAG,
           "clock": "HIP events around one call (forward + backward), variants alternating", "shapes": rows}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
