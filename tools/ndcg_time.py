"""NDCG from graded label overlap: what the two kernels cost, against what a user of the previous commit could have run on the
device for the same number, in ONE process, alternating.

    python tools/ndcg_time.py [--out profiles/ndcg.txt] [--rounds 7] [--calls 5] [--shapes c1,c1x3,c3]

Per shape the HIP-event time per evaluation of
  (h) label_overlap_hist                 -- the per-query overlap histogram, one pass over the label words
  (w) ndcg_at_ks                         -- the walk over given lists with a given histogram: DCG and ideal DCG at every cut-off
  (m) hamming_topk + (h) + (w)           -- the whole metric from packed codes and labels
  (t) torch composition                  -- hamming_topk, then per query chunk ql @ rl.T, 2^Rel - 1 in fp64, a gather along the
                                            list and a descending sort of all N gains for the ideal (the reference's steps, on
                                            the device, in chunks so that the [chunk, N] temporaries fit)
  (l) hamming_topk alone, for scale
c3 (5000 x 117,218 labels, 80 classes) measures the histogram only, against (ti) the ideal-DCG part of the torch composition
(ql @ rl.T and the descending sort, in chunks).  Alternating rounds after a clock warm-up; per path median and [min, max].
(m) and (t) are checked equal to (4 k + 2) 2^-53 before anything is timed.  No threshold is asserted: the numbers are the result."""
import argparse
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import synth  # noqa: E402
from wvhash.engine import hamming as H  # noqa: E402
from wvhash.engine import ndcg as ND  # noqa: E402

SHAPES = {"c1": (2048, 25000, 64, 38, 0.10, (1000,)),
          "c1x3": (2048, 25000, 64, 38, 0.10, (100, 1000, 5000)),
          "c3": (5000, 117218, 128, 80, 0.036, None)}            # histogram only


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # ms per evaluation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--clock-calls", type=int, default=200, help="untimed histogram calls before anything is measured")
    ap.add_argument("--shapes", default="c1,c1x3,c3")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds, ms per evaluation: median [min, max] "
         f"({args.calls} evaluations per round; torch paths 1)")
    warmed = False
    for name in args.shapes.split(","):
        Q, N, nbits, classes, p, ks = SHAPES[name]
        ql, rl = synth.multi_hot_labels(Q, classes, p, 1), synth.multi_hot_labels(N, classes, p, 2)
        qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
        qlf, rlf = ql.cuda().float(), rl.cuda().float()

        def hist():
            return H.label_overlap_hist(qlp, rlp)

        if not warmed:
            for _ in range(args.clock_calls):
                hist()
            torch.cuda.synchronize()
            warmed = True
        chunk = max(1, (48 << 20) // (8 * N))                    # [chunk, N] fp64 temporaries of 48 MB

        def torch_ideal(kmax=None):
            out = []
            for s in range(0, Q, chunk):
                G = torch.exp2((qlf[s:s + chunk] @ rlf.t()).double()) - 1
                best = torch.sort(G, dim=1, descending=True)[0]
                out.append(best if kmax is None else best[:, :kmax])
            return out

        if ks is None:
            paths = (("(h)  label_overlap_hist", hist, args.calls), ("(ti) torch: ql @ rl.T + descending sort", torch_ideal, 1))
            h = hist()
            G = torch.exp2((qlf[:8] @ rlf.t()).double()) - 1     # the histogram describes the sorted gains
            assert torch.equal(torch.bincount((qlf[3] @ rlf.t()).long(), minlength=h.shape[1]).int(), h[3]) and G.shape[1] == N
        else:
            q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
            qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
            prep = H.PreparedDB(rp, nbits)
            kmax = max(ks)
            idx0 = H.hamming_topk(qp, prep, nbits, kmax, want_dist=False)[0]
            h0 = hist()
            D = torch.log2(2.0 + torch.arange(kmax, device="cuda", dtype=torch.float64))
            cols = torch.tensor([k - 1 for k in ks], device="cuda")

            def lists():
                return H.hamming_topk(qp, prep, nbits, kmax, want_dist=False)[0]

            def walk():
                return H.ndcg_at_ks(idx0, qlp, rlp, ks, hist=h0)

            def metric():
                return ND.ndcg_from_sums(*H.ndcg_at_ks(lists(), qlp, rlp, ks, hist=hist()))

            def torch_metric():
                idx = lists().long()
                total = torch.zeros(len(ks), dtype=torch.float64, device="cuda")
                for s in range(0, Q, chunk):
                    G = torch.exp2((qlf[s:s + chunk] @ rlf.t()).double()) - 1
                    dcg = (torch.gather(G, 1, idx[s:s + chunk]) / D).cumsum(1)[:, cols]
                    best = (torch.sort(G, dim=1, descending=True)[0][:, :kmax] / D).cumsum(1)[:, cols]
                    total += torch.where(best > 0, dcg / best.clamp(min=1e-300), torch.zeros_like(dcg)).sum(0)
                return total / Q

            ours, theirs = metric(), torch_metric()
            assert float((ours - theirs).abs().max()) <= (4 * kmax + 2) * 2.0 ** -53, (ours, theirs)
            paths = (("(h)  label_overlap_hist", hist, args.calls), ("(w)  ndcg_at_ks", walk, args.calls),
                     ("(m)  topk + hist + walk", metric, args.calls), ("(t)  torch composition", torch_metric, 1),
                     ("(l)  hamming_topk alone", lists, args.calls))
        times = {label: [] for label, _, _ in paths}
        for _ in range(args.rounds):
            for label, fn, calls in paths:
                times[label].append(timed(fn, calls))
        emit(f"{name}: {Q} queries x {N} rows, {classes} classes" + (f", {nbits} bit, k = {', '.join(str(k) for k in ks)}" if ks else
                                                                   " (labels only)"))
        for label, _, _ in paths:
            t = times[label]
            emit(f"  {label:<42} {statistics.median(t):9.3f} [{min(t):8.3f}, {max(t):8.3f}]")
        med = {label: statistics.median(t) for label, t in times.items()}
        if ks is None:
            emit(f"  (ti) / (h) = {med[paths[1][0]] / med[paths[0][0]]:.1f}")
        else:
            emit(f"  (t) / (m) = {med[paths[3][0]] / med[paths[2][0]]:.1f}   (m) - (l) = {med[paths[2][0]] - med[paths[4][0]]:.3f} ms")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
