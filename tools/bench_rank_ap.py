"""The rank-approximation AP losses in ONE run: loss + backward to the scores through the fused path (wv_rank_ap behind
wvhash.losses' autograd Function) against the plain PyTorch path of the SAME module on the same GPU -- the reference's op
sequence: [B, B, B] tensors for a square input, a Python loop over the queries for a rectangular one -- for SupAP as
configured (tau 0.01, rho 100, offset 1.44, delta 0.05) and SmoothAP(tau 0.01), at square B = 96 (the configured batch), 256,
512 and at 96 x 4096 (general form: a batch against a memory bank).

    python tools/bench_rank_ap.py [--out profiles/rank_ap.json] [--rounds 6] [--calls 5]

One call = module(scores, target) then .backward() into scores.grad: what train_step pays per step for the loss (the 0 / 1
target check with its synchronise included on the fused side).  Scores are inner products of unit vectors (D = 64), targets
the label matrix of 38 classes at p = 0.08 with no empty row.  Per shape, after a warm-up of both variants, variants
alternating inside every round, median [min, max] over rounds x calls single calls, HIP events around the call; the peak
of torch.cuda.max_memory_allocated over one call of each variant, above what was allocated before it.  The two paths'
numbers are compared first (value relative, gradient norm-wise).  Prints one JSON row per shape; --out writes them.
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import losses as L  # noqa: E402
from _timing import fused_against_plain  # noqa: E402

SHAPES = ((96, 96), (256, 256), (512, 512), (96, 4096))
D, CLASSES, P_TAG = 64, 38, 0.08


def modules():
    return {"SupAP": lambda: L.SupAP(tau=0.01, rho=100.0, offset=1.44, delta=0.05), "SmoothAP": lambda: L.SmoothAP(tau=0.01)}


def make_inputs(B, M):
    g = torch.Generator().manual_seed(B * 10007 + M)
    rows = max(B, M)
    emb = F.normalize(torch.randn(rows, D, generator=g), dim=1)
    lab = (torch.rand(rows, CLASSES, generator=g) < P_TAG).float()
    lab[lab.sum(1) == 0, 0] = 1
    target = ((lab[:B] @ lab[:M].t()) > 0).float()
    return (emb[:B] @ emb[:M].t()).cuda().requires_grad_(True), target.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_ap: needs the GPU (a time measured elsewhere says nothing about it)")
    lines = []
    for B, M in SHAPES:
        scores, target = make_inputs(B, M)
        per_loss = {}
        for kind, make in modules().items():
            fused, plain = make(), make()
            fused.fused, plain.fused = True, False

            def step(module):
                scores.grad = None
                val = module(scores, target)
                val.backward()
                return val.detach(), scores.grad

            per_loss[kind] = fused_against_plain(lambda: step(fused), lambda: step(plain), 3, args.rounds, args.calls, memory=True)
            del fused, plain
            scores.grad = None
            torch.cuda.empty_cache()
        row = {"what": "loss (1 - mAP) + backward to the scores: wv_rank_ap behind the autograd Function (fused) against the "
                       "plain PyTorch path of the same module",
               "device": torch.cuda.get_device_name(0), "B": B, "M": M, "form": "quick" if B == M else "general",
               "positives_per_row": round(float(target.sum(1).mean()), 1),
               "clock": "HIP events around one call (forward + backward), variants alternating", "losses": per_loss}
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
