"""Head-only timing of the bf16 matrix-core path against the fp32 path, in ONE process, alternating.

    python tools/head_bf16_time.py [--out profiles/head_bf16.txt] [--rounds 7] [--calls 20]

For B in {200, 1000, 2048, 4096} x Nq in {4, 8} (E = 384, 4 band tokens, 8 heads) and fp32- / bf16-typed band features:
HIP-event time per call of `band_attn_pool` with matrix_dtype=None (the fp32 head: one-launch front where the batch fills
the chip) and matrix_dtype="bf16", measured in alternating rounds after a clock warm-up (as bench.py's clock_steps: the
GPU clock ramps after idle).  Per row: median and [min, max] over the rounds of both paths, the ratio, and the bf16
path's achieved FLOP/s against the 2.5 PFLOP/s bf16 matrix peak.  The prepare step (once per parameter update) is timed
separately.  --trace runs every configuration ten times per path and nothing else (for rocprofv3 --kernel-trace --stats;
--shapes 2048x4 keeps the kernel statistics to one shape)."""
import argparse
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import synth  # noqa: E402
from wvhash.models import get_fusion_head  # noqa: E402
from wvhash.models._prepared import PreparedCache  # noqa: E402
from wvhash.models.fusion import band_attn_pool  # noqa: E402

E, HEADS, S = 384, 8, 4
PEAK_BF16 = 2.5e15


def make_head(nq):
    head = get_fusion_head({"type": "cross_attention_advanced", "output_dim": E, "num_queries": nq, "num_heads": HEADS}, [E] * S)
    head.load_state_dict(synth.head_state(E, nq, "concat", seed=nq))
    return head.cuda().eval()


def call(head, feats, matrix_dtype, cache=None):
    return band_attn_pool(feats, head.effective_queries(), head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2],
                          head.out_proj, False, cache or head._prepared, head._query_key(), matrix_dtype=matrix_dtype)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per call


def flops(B, nq):
    rows = B * nq
    return 2.0 * (S * B * 2 * E * E + rows * E * E + 2 * rows * 4 * E * E + B * E * nq * E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--clock-calls", type=int, default=400, help="untimed calls before anything is measured")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shapes", default="200x4,1000x4,2048x4,4096x4,200x8,1000x8,2048x8,4096x8", help="B x Nq list")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")]
    heads = {nq: make_head(nq) for nq in sorted({4, 8} | {nq for _, nq in shapes})}
    with torch.no_grad():
        warm = [f.cuda() for f in synth.band_features(2048, E, seed=1)]
        for _ in range(args.clock_calls):
            call(heads[4], warm, None)
        torch.cuda.synchronize()
        emit(f"# {torch.cuda.get_device_name(0)}; E={E} heads={HEADS} tokens={S}; {args.rounds} alternating rounds of {args.calls} calls, "
             f"us per call: median [min, max]")
        emit(f"{'B':>5} {'Nq':>2} {'feats':>5} | {'fp32 head':>24} | {'bf16 head':>24} | {'fp32/bf16':>9} | {'bf16 TFLOP/s':>12} {'of peak':>7}")
        for B, nq in shapes:
            if True:
                base = synth.band_features(B, E, seed=B)
                for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                    # one [S, B, E] buffer, as the backbones write it: both paths read it in place when the dtype allows
                    buf = torch.stack(base).cuda().to(dt).contiguous()
                    feats = list(buf.unbind(0))
                    f32 = lambda: call(heads[nq], feats, None)
                    b16 = lambda: call(heads[nq], feats, "bf16")
                    for _ in range(10 if args.trace else 3):
                        f32(), b16()
                    if args.trace:
                        continue
                    t32, t16 = [], []
                    for _ in range(args.rounds):
                        t32.append(timed(f32, args.calls))
                        t16.append(timed(b16, args.calls))
                    m32, m16 = statistics.median(t32), statistics.median(t16)
                    tf = flops(B, nq) / (m16 * 1e-6)
                    emit(f"{B:>5} {nq:>2} {name:>5} | {m32:8.1f} [{min(t32):6.1f}, {max(t32):6.1f}] | {m16:8.1f} [{min(t16):6.1f}, {max(t16):6.1f}] "
                         f"| {m32 / m16:9.2f} | {tf / 1e12:12.1f} {100 * tf / PEAK_BF16:6.1f}%")
        if not args.trace:
            for nq in (4, 8):
                head = heads[nq]
                feats = [f.cuda() for f in synth.band_features(64, E, seed=2)]

                def prep():
                    call(head, feats, "bf16", PreparedCache())     # a fresh cache: the blob is built in this call
                run = timed(lambda: call(head, feats, "bf16"), args.calls)
                emit(f"prepare (bf16 weight copy + query projection), Nq={nq}: {timed(prep, args.calls) - run:.1f} us per parameter update")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
