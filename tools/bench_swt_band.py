"""The single-band SWT kernel against the four-band kernel, in ONE run: 2048 x 224 x 224 x 3 uint8 images (shape c1), for
db2 level 3 -> fp32, db2 level 3 -> bf16 and haar level 1 -> fp32.

    python tools/bench_swt_band.py [--out profiles/swt_band.json] [--batch 2048] [--rounds 7] [--calls 4]

Per configuration and band (0..3 = cA, cH, cV, cD), timed with HIP events around single launches after a warm-up, variants
alternating inside every round, median over rounds x calls launches (>= 20):
  band_ms               wv_swt2d_band_forward: the one band computed and written
  four_band_slice_ms    wv_swt2d_forward followed by [:, :, band].contiguous(): the only way to the same tensor before
and per configuration
  four_band_ms          wv_swt2d_forward alone, same rounds
  equal                 every band equals the slice (checked before anything is timed)
Rates: images / s, and the fraction of 8 TB/s (HBM peak) the ALGORITHMIC bytes take -- input read once, output written once:
150,528 + 602,112 = 752,640 B / image for one fp32 band, 150,528 + 301,056 = 451,584 B for one bf16 band, 2,558,976 /
1,354,752 B for four bands.  Prints one JSON row.
"""
import argparse
import json
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import synth  # noqa: E402
from wvhash.transforms import swt2d, swt2d_band  # noqa: E402

H = W = 224
HBM_PEAK = 8e12
CONFIGS = [("db2", 3, torch.float32), ("db2", 3, torch.bfloat16), ("haar", 1, torch.float32)]


def algo_bytes(bands, dtype):
    return 3 * H * W + bands * 3 * H * W * (4 if dtype == torch.float32 else 2)


def one_launch_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rate(B, ms, nbytes):
    return {"ms": round(ms, 4), "images_per_s": round(B / ms * 1e3, 1), "hbm_fraction": round(B * nbytes / (ms * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swt_band: needs the GPU (a rate measured elsewhere says nothing about it)")
    B = args.batch
    tile = torch.from_numpy(synth.natural_images(64, H, W, seed=1)).permute(0, 3, 1, 2).contiguous()
    x = tile.repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous().cuda()            # planar uint8 [B, 3, 224, 224]
    configs = []
    for wl, lev, dt in CONFIGS:
        full = torch.empty((B, 3, 4, H, W), dtype=dt, device="cuda")
        one = torch.empty((B, 3, H, W), dtype=dt, device="cuda")
        swt2d(x, wl, lev, out_dtype=dt, out=full)
        equal = all(bool(torch.equal(swt2d_band(x, wl, lev, b, out_dtype=dt, out=one), full[:, :, b])) for b in range(4))
        variants = {"four": lambda: swt2d(x, wl, lev, out_dtype=dt, out=full)}
        for b in range(4):
            variants[f"band{b}"] = lambda b=b: swt2d_band(x, wl, lev, b, out_dtype=dt, out=one)
            variants[f"slice{b}"] = lambda b=b: one.copy_(swt2d(x, wl, lev, out_dtype=dt, out=full)[:, :, b])
        for _ in range(5):                                                      # warm-up: code objects, clocks
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):                                            # alternating
            for k, fn in variants.items():
                ms[k] += [one_launch_ms(fn) for _ in range(args.calls)]
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = {"wavelet": wl, "level": lev, "out": "f32" if dt == torch.float32 else "bf16", "equal": equal,
               "launches_per_variant": args.rounds * args.calls,
               "four_band": dict(rate(B, med["four"], algo_bytes(4, dt)), ms_min=round(min(ms["four"]), 4)), "bands": []}
        for b in range(4):
            r = rate(B, med[f"band{b}"], algo_bytes(1, dt))
            r.update(band=b, ms_min=round(min(ms[f"band{b}"]), 4), four_band_slice_ms=round(med[f"slice{b}"], 4),
                     below_four_band=bool(med[f"band{b}"] < med["four"]),
                     speedup_over_four_band=round(med["four"] / med[f"band{b}"], 3),
                     speedup_over_slice=round(med[f"slice{b}"] / med[f"band{b}"], 3))
            row["bands"].append(r)
        configs.append(row)
        del full, one
        torch.cuda.empty_cache()
    row = {"what": "wv_swt2d_band_forward against wv_swt2d_forward, planar uint8 in", "device": torch.cuda.get_device_name(0),
           "batch": B, "shape": [H, W, 3], "algorithmic_bytes_per_image": {"band_f32": algo_bytes(1, torch.float32),
           "band_bf16": algo_bytes(1, torch.bfloat16), "four_f32": algo_bytes(4, torch.float32),
           "four_bf16": algo_bytes(4, torch.bfloat16)}, "configs": configs}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
