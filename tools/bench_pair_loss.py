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
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import losses as L  # noqa: E402
from _timing import fused_against_plain  # noqa: E402

BATCHES, D, CLASSES, P_TAG = (64, 96, 128, 1024), 64, 38, 0.08


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

            rows.append({"loss": kind, "B": B, "D": D,
                         **fused_against_plain(lambda: step(fused), lambda: step(plain), 5, args.rounds, args.calls)})
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
