"""Cost of the attention maps next to the head's own forward, in ONE process, alternating.

    python tools/head_attn_maps_time.py [--out profiles/head_attn_maps.txt] [--rounds 7] [--calls 20]

At B = 2048, S = 4, Nq = 4, E = 384, 8 heads: HIP-event time per call of wv_band_attn_maps with all four outputs (probs,
probs_mean, scores, attn_out; workspace and outputs allocated once) and of wv_band_attn_pool with its separate launches
(WV_HEAD_FRONT=0 on the diagnostic library: the stage sequence the maps share their first stages with), measured in
alternating rounds after a clock warm-up.  Also the maps without attn_out (K projected alone, no out-projection).  The maps
are a diagnostic path: there is no target, the figures are for the record."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path[:0] = [".", "image-retrieval-wavelet_amd"]
from wvhash import _lib, synth  # noqa: E402
from wvhash.models import fusion, get_fusion_head  # noqa: E402

E, HEADS, S, NQ = 384, 8, 4, 4


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--clock-calls", type=int, default=400, help="untimed calls before anything is measured")
    args = ap.parse_args()
    B = args.batch
    os.environ["WV_HEAD_FRONT"] = "0"
    head = get_fusion_head({"type": "cross_attention_advanced", "output_dim": E, "num_queries": NQ, "num_heads": HEADS}, [E] * S)
    head.load_state_dict(synth.head_state(E, NQ, "concat", seed=NQ))
    head = head.cuda().eval()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    with torch.no_grad(), _lib.diagnostic() as lib:
        feats = torch.stack(synth.band_features(B, E, seed=B)).cuda().contiguous()            # [S, B, E]
        q_eff = head.effective_queries().detach().float().reshape(-1, E).contiguous()
        p, keep = fusion._head_params(S, E, q_eff, head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2], head.out_proj, False)
        new = lambda *shape: torch.empty(shape, device="cuda")
        probs, mean, scores, attn_out, pooled = new(B, HEADS, NQ, S), new(B, NQ, S), new(B, HEADS, NQ, S), new(B, NQ, E), new(B, E)
        ws_m = torch.empty(lib.wv_band_attn_maps_workspace_bytes(ctypes.byref(p), B), dtype=torch.uint8, device="cuda")
        ws_p = torch.empty(lib.wv_band_attn_pool_workspace_bytes(ctypes.byref(p), B), dtype=torch.uint8, device="cuda")
        st = _lib.stream_ptr()

        def maps(with_out=True):
            _lib.check(lib.wv_band_attn_maps(ctypes.byref(p), _lib.ptr(feats), _lib.WV_TOKENS_SBE, B, _lib.ptr(probs), _lib.ptr(mean),
                                             _lib.ptr(scores), _lib.ptr(attn_out if with_out else None), _lib.ptr(ws_m),
                                             ctypes.c_size_t(ws_m.numel()), st), "wv_band_attn_maps")

        def pool():
            _lib.check(lib.wv_band_attn_pool(ctypes.byref(p), _lib.ptr(feats), B, _lib.ptr(pooled), _lib.ptr(ws_p),
                                             ctypes.c_size_t(ws_p.numel()), st), "wv_band_attn_pool")

        for _ in range(args.clock_calls):
            pool()
        for _ in range(3):
            maps(), maps(False), pool()
        torch.cuda.synchronize()
        t = {"maps": [], "maps_no_out": [], "pool": []}
        for _ in range(args.rounds):
            t["maps"].append(timed(maps, args.calls))
            t["pool"].append(timed(pool, args.calls))
            t["maps_no_out"].append(timed(lambda: maps(False), args.calls))
        emit(f"# {torch.cuda.get_device_name(0)}; B={B} S={S} Nq={NQ} E={E} heads={HEADS}; {args.rounds} alternating rounds of "
             f"{args.calls} calls, us per call: median [min, max]")
        for name, label in (("maps", "wv_band_attn_maps, all four outputs"),
                            ("maps_no_out", "wv_band_attn_maps, probs + probs_mean + scores"),
                            ("pool", "wv_band_attn_pool, WV_HEAD_FRONT=0 (no q_proj, no prepared blob)")):
            v = t[name]
            emit(f"{label:<62} {statistics.median(v):8.1f} [{min(v):6.1f}, {max(v):6.1f}]")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
