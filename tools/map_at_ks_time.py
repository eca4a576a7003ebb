"""mAP at several cut-offs: what one multi-cut call costs against the ways to get the same numbers, in ONE process, alternating.

    python tools/map_at_ks_time.py [--out profiles/map_at_ks.txt] [--rounds 7] [--calls 5] [--shapes small,c1,c3]

Per shape the HIP-event time per evaluation (all cut-offs of the shape answered) of
  (a)  hamming_topk at k_max + map_at_k per k      -- the [Q, k_max] lists are written, then read and their labels gathered
                                                     once per k (what evaluate_multi_k did before the multi-cut entry points)
  (a') hamming_topk at k_max + map_at_ks           -- the lists are written, read once (evaluate_multi_k with a k-NN metric)
  (b)  hamming_map_at_k per k                      -- one fused ranking + AP pass per cut-off, no list
  (c)  hamming_map_at_ks                           -- ONE fused pass, no list
and, for scale, (k) hamming_map_at_k at k_max alone: (c) walks a list of the same length.
Measured in alternating rounds after a clock warm-up (the GPU clock ramps after idle); per path median and [min, max] over the
rounds.  Shapes: small = 2048 queries x 5,000 rows, 64 bit, 38 classes, k = 100, 1000, 5000; c1 = 2048 queries x 25,000 rows, 64 bit, 38 classes, k = 1000, 5000, 25000; c3 = 5000 x 117,218, 128 bit, 80
classes, k = 5000, 117218 (three virtual shards; its calls read one host scalar for the prefix length, which is inside the
bracket as it is inside every real call).

    python tools/map_at_ks_time.py --single [--rounds 7] [--calls 20]

times the single-cut entry points alone, for comparing two builds of the library (run it in fresh processes, alternating):
  (l) map_at_k on resident lists, k = 5000, at small / c1 / c3 (one label word, one, two)
  (m) merge_relbits_map on resident wires of G = 8 shards emulated on one GPU: 2048 queries, k = 5000 of 25,000 rows, 64 bit;
      625 queries, k = 117,218 of 117,218 rows, 128 bit."""
import argparse
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import synth  # noqa: E402
from wvhash.engine import hamming as H  # noqa: E402

SHAPES = {"small": (2048, 5000, 64, 38, 0.10, (100, 1000, 5000)),      # 20 rows per thread: the kernels' smallest register bucket pair
          "c1": (2048, 25000, 64, 38, 0.10, (1000, 5000, 25000)),
          "c3": (5000, 117218, 128, 80, 0.036, (5000, 117218))}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # ms per evaluation


MERGES = ((2048, 25000, 64, 38, 0.10, 5000), (625, 117218, 128, 80, 0.036, 117218))


def single_cut(args, emit):
    """(l) and (m) of the module header: one kernel launch per evaluation, inputs resident."""
    def report(label, fn):
        t = [timed(fn, args.calls) for _ in range(args.rounds)]
        emit(f"  {label:<58} {statistics.median(t):9.4f} [{min(t):8.4f}, {max(t):8.4f}]")

    for name in ("small", "c1", "c3"):
        Q, N, nbits, classes, p, _ = SHAPES[name]
        ql, rl = synth.multi_hot_labels(Q, classes, p, 1), synth.multi_hot_labels(N, classes, p, 2)
        q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
        qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
        idx, _ = H.hamming_topk(H.pack_codes(q.cuda()), H.pack_codes(r.cuda()), nbits, 5000, want_dist=False)
        for _ in range(args.clock_calls):
            H.map_at_k(idx, qlp, rlp)
        report(f"(l) map_at_k {name}: {Q} x k=5000, {qlp.shape[1]} label word(s)", lambda: H.map_at_k(idx, qlp, rlp))
    G = 8
    for Q, N, nbits, classes, p, k in MERGES:
        ql, rl = synth.multi_hot_labels(Q, classes, p, 1), synth.multi_hot_labels(N, classes, p, 2)
        q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
        qp, rp, qlp, rlp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda()), H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
        per = (N + G - 1) // G
        send = min(k, per)
        wires = torch.zeros((G, Q, H.relbits_wire_words(send, nbits)), dtype=torch.int64, device="cuda")
        for g in range(G):
            lo, hi = g * per, min(N, (g + 1) * per)
            got = H.hamming_shard_relbits(qp, H.PreparedDB(rp[lo:hi].contiguous(), nbits), H.PreparedLabels(rlp[lo:hi].contiguous()), qlp,
                                          nbits, min(send, hi - lo), wire=wires[g], kin=send)
            assert got is not None
        idx, _ = H.hamming_topk(qp, rp, nbits, k, want_dist=False)
        want = H.map_at_k(idx, qlp, rlp)
        got = H.merge_relbits_map(wires, send, k, nbits)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        del idx
        for _ in range(args.clock_calls):
            H.merge_relbits_map(wires, send, k, nbits)
        report(f"(m) merge_relbits_map G=8: {Q} x k={k}, {nbits} bit", lambda: H.merge_relbits_map(wires, send, k, nbits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", action="store_true", help="time map_at_k and merge_relbits_map alone (module header)")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--clock-calls", type=int, default=300, help="untimed fused c1-sized calls before anything is measured")
    ap.add_argument("--shapes", default="small,c1,c3")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.calls} evaluations, ms per evaluation: median [min, max]")

    def finish():
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    if args.single:
        single_cut(args, emit)
        return finish()
    warmed = False
    for name in args.shapes.split(","):
        Q, N, nbits, classes, p, ks = SHAPES[name]
        ql, rl = synth.multi_hot_labels(Q, classes, p, 1), synth.multi_hot_labels(N, classes, p, 2)
        q, r = synth.structured_codes(ql, nbits, 3, 4), synth.structured_codes(rl, nbits, 3, 5)
        qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
        qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
        prep, labels = H.PreparedDB(rp, nbits), H.PreparedLabels(rlp)
        kmax = max(ks)

        def lists_then_per_k():
            idx, _ = H.hamming_topk(qp, prep, nbits, kmax, want_dist=False)
            return [H.map_at_k(idx, qlp, rlp, k=k)[0] for k in ks]

        def lists_then_once():
            idx, _ = H.hamming_topk(qp, prep, nbits, kmax, want_dist=False)
            return H.map_at_ks(idx, qlp, rlp, ks)[0]

        def fused_per_k():
            return [H.hamming_map_at_k(qp, prep, labels, qlp, nbits, k)[0] for k in ks]

        def fused_once():
            return H.hamming_map_at_ks(qp, prep, labels, qlp, nbits, ks)[0]

        def fused_kmax():
            return H.hamming_map_at_k(qp, prep, labels, qlp, nbits, kmax)[0]

        paths = (("(a)  topk + map_at_k per k", lists_then_per_k), ("(a') topk + map_at_ks", lists_then_once),
                 ("(b)  fused per k", fused_per_k), ("(c)  fused, all k at once", fused_once), ("(k)  fused at k_max alone", fused_kmax))
        if not warmed:
            for _ in range(args.clock_calls):
                fused_kmax()
            torch.cuda.synchronize()
            warmed = True
        want = torch.stack(fused_per_k(), dim=1)                 # every path computes the same numbers
        for label, fn in paths[:4]:
            got = fn()
            got = torch.stack(got, dim=1) if isinstance(got, list) else got
            assert torch.equal(got, want), label
        times = {label: [] for label, _ in paths}
        for _ in range(args.rounds):
            for label, fn in paths:
                times[label].append(timed(fn, args.calls))
        emit(f"{name}: {Q} queries x {N} rows, {nbits} bit, {classes} classes, k = {', '.join(str(k) for k in ks)}")
        for label, _ in paths:
            t = times[label]
            emit(f"  {label:<28} {statistics.median(t):9.3f} [{min(t):8.3f}, {max(t):8.3f}]")
        med = {label: statistics.median(t) for label, t in times.items()}
        emit(f"  (c) / (b) = {med[paths[3][0]] / med[paths[2][0]]:.3f}   (c) / (a) = {med[paths[3][0]] / med[paths[0][0]]:.3f}   "
             f"(c) / (k) = {med[paths[3][0]] / med[paths[4][0]]:.3f}")
    finish()


if __name__ == "__main__":
    main()
