"""Radius histograms (precision / recall by Hamming radius): what one call costs against the ways to get the same two tables,
in ONE process, alternating.

    python tools/radius_time.py [--out profiles/radius_hist.txt] [--rounds 7] [--calls 5] [--shapes c1,c3]

Per shape the HIP-event time per evaluation (both tables [Q, nbits + 2] on the device) of
  (h) hamming_hist alone                         -- the floor: the same distance pass, no labels, one table only
  (r) hamming_radius_hist                        -- the new call
  (m) hamming_dist + relevance matrix + scatter_add  -- what a user did before: the [Q, N] distance bytes, ql @ rl.T > 0 and
                                                    two scatter_add in torch, chunked over queries so the temporaries fit
  (l) hamming_topk at k = N + hit_prefix         -- lists and running hit counts of the whole ranking, the tables read off
                                                    them (c1 only: at c3 the lists alone are 2.35 GB)
Every path's tables are compared with (r)'s before anything is timed.  Alternating rounds after a clock warm-up (the GPU clock
ramps after idle); per path median and [min, max] over the rounds.  Shapes: c1 = 2048 queries x 25,000 rows, 64 bit, 38
classes; c3 = 5000 x 117,218, 128 bit, 80 classes (four virtual shards: (h) and (r) are sums of per-part calls)."""
import argparse
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import synth  # noqa: E402
from wvhash.engine import hamming as H  # noqa: E402

SHAPES = {"c1": (2048, 25000, 64, 38, 0.10, True),
          "c3": (5000, 117218, 128, 80, 0.036, False)}


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
    ap.add_argument("--clock-calls", type=int, default=300, help="untimed calls of (r) before anything is measured")
    ap.add_argument("--chunk", type=int, default=256, help="queries per chunk of path (m)")
    ap.add_argument("--shapes", default="c1,c3")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.calls} evaluations, ms per evaluation: median [min, max]")
    warmed = False
    for name in args.shapes.split(","):
        Q, N, nbits, classes, p, with_lists = SHAPES[name]
        ql, rl = synth.multi_hot_labels(Q, classes, p, 1), synth.multi_hot_labels(N, classes, p, 2)
        q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
        qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
        qlg, rlg = ql.cuda(), rl.cuda()
        qlp, rlp = H.pack_labels(qlg), H.pack_labels(rlg)
        prep, labels = H.PreparedDB(rp, nbits), H.PreparedLabels(rlp)

        def hist_only():
            if prep.parts:
                return sum(H.hamming_hist(qp, part, nbits) for part in prep.parts)
            return H.hamming_hist(qp, prep, nbits)

        def radius():
            return H.hamming_radius_hist(qp, prep, labels, qlp, nbits)

        def matrices():
            cnt = torch.zeros((2, Q, nbits + 2), dtype=torch.int64, device="cuda")
            for s in range(0, Q, args.chunk):
                d = H.hamming_dist(qp[s:s + args.chunk], prep, nbits).long() + 1
                rel = (qlg[s:s + args.chunk] @ rlg.t() > 0).long()
                cnt[0, s:s + args.chunk].scatter_add_(1, d, torch.ones_like(d))
                cnt[1, s:s + args.chunk].scatter_add_(1, d, rel)
            cum = cnt.cumsum(2).int()
            return cum[0], cum[1]

        def lists():
            idx, dist = H.hamming_topk(qp, prep, nbits, N)
            hits = H.hit_prefix(idx, qlp, rlp)
            cnt = torch.zeros((Q, nbits + 2), dtype=torch.int64, device="cuda")
            for s in range(0, Q, args.chunk):
                d = dist[s:s + args.chunk].long() + 1
                cnt[s:s + args.chunk].scatter_add_(1, d, torch.ones_like(d))
            cum = cnt.cumsum(1)
            cumrel = torch.where(cum > 0, torch.gather(hits, 1, (cum - 1).clamp(min=0)), torch.zeros_like(hits[:, :1]))
            return cum.int(), cumrel.int()

        paths = [("(h) hamming_hist alone", hist_only), ("(r) hamming_radius_hist", radius), ("(m) dist + relevance + scatter_add", matrices)]
        if with_lists:
            paths.append(("(l) topk at k = N + hit_prefix", lists))
        if not warmed:
            for _ in range(args.clock_calls):
                radius()
            torch.cuda.synchronize()
            warmed = True
        want = radius()                                          # every path computes the same tables
        assert torch.equal(hist_only(), want[0]), "(h)"
        for label, fn in paths[2:]:
            got = fn()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), label
        times = {label: [] for label, _ in paths}
        for _ in range(args.rounds):
            for label, fn in paths:
                times[label].append(timed(fn, args.calls))
        emit(f"{name}: {Q} queries x {N} rows, {nbits} bit, {classes} classes" + (f", {len(prep.parts)} virtual shards" if prep.parts else ""))
        for label, _ in paths:
            t = times[label]
            emit(f"  {label:<38} {statistics.median(t):9.3f} [{min(t):8.3f}, {max(t):8.3f}]")
        med = {label: statistics.median(t) for label, t in times.items()}
        emit(f"  (r) / (h) = {med[paths[1][0]] / med[paths[0][0]]:.3f}   (r) / (m) = {med[paths[1][0]] / med[paths[2][0]]:.4f}" +
             (f"   (r) / (l) = {med[paths[1][0]] / med[paths[3][0]]:.4f}" if with_lists else ""))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
