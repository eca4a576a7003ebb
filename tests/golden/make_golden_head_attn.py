#!/usr/bin/env python3
"""Regenerates tests/golden/head_attn_golden.npz.  Run in the BUILD container only (needs /root/reference):
    python tests/golden/make_golden_head_attn.py

What the file pins: what the REFERENCE's own fusion-head modules hand to an observer of their `attn` submodule in eval mode
-- the per-head softmax weights and the attention output -- with need_weights=True, average_attn_weights=False forced on the
module's forward the way studies/measure_attention_collapse.py forces it (an instance-level `forward` that overrides the
two keywords), captured by a forward hook.  Per case:
  <case>/probs     [B, H, Nq, 4]  output[1] of the hooked call
  <case>/attn_out  [B, Nq, E]     output[0]
  <case>/meta      E, heads, Nq, B, seed, mean read-out, decoupled, factor;  <case>/qscale, <case>/sha as in head_golden.npz
Cases: the seven of make_golden.py::HEAD_CASES (same seeds and batch sizes, weights from wvhash.synth.head_state), and
adv_e384_nq4, adv_e64_nq4, adv_e384_nq8 again at B = 6 with `query_tokens` multiplied by 4 (`<case>_x4`: attention that is
neither uniform nor one-hot) and by 100 (`<case>_x100`: scores of +-130 ... +-210, where expf without the max subtraction
overflows).  The factor multiplies the state_dict's query_tokens before it is loaded; the stored SHA is of the unscaled
weights.  Fixtures are data only: inputs are regenerated from seeds, outputs are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (sets sys.path for oracle / wvhash)
from wvhash import synth  # noqa: E402

SCALED = ("adv_e384_nq4", "adv_e64_nq4", "adv_e384_nq8")
FACTORS = (4, 100)
SCALED_B = 6


def cases():
    """name, fusion type, E, heads, Nq, extra fusion_config, B, seed, factor"""
    out = [c + (1,) for c in mg.HEAD_CASES]
    by_name = {c[0]: c for c in mg.HEAD_CASES}
    for factor in FACTORS:
        for n in SCALED:
            name, ftype, E, heads, nq, extra, _, seed = by_name[n]
            out.append((f"{name}_x{factor}", ftype, E, heads, nq, extra, SCALED_B, seed, factor))
    return out


def force_per_head(attn):
    original = attn.forward

    def forced(*args, **kwargs):
        kwargs["need_weights"] = True
        kwargs["average_attn_weights"] = False
        return original(*args, **kwargs)

    attn.forward = forced
    return lambda: setattr(attn, "forward", original)


def main():
    mda = mg.load_reference_heads()
    out = {}
    for name, ftype, E, heads, nq, extra, B, seed, factor in cases():
        cfg = {"type": ftype, "output_dim": E, "num_heads": heads, "dropout": 0.1, "num_queries": nq,
               "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
        cfg.update(extra)
        head = mda.get_fusion_head(cfg, [E] * 4).eval()
        pool = "mean" if extra.get("query_pool") == "mean" else "concat"
        qs = extra.get("query_scale_init")
        sd = synth.head_state(E, nq, pool, seed, query_scale=qs)
        sha = synth.state_sha(sd)
        sd["query_tokens"] = sd["query_tokens"] * float(factor)
        head.load_state_dict(sd, strict=True)
        feats = synth.band_features(B, E, seed + 1000)
        captured = []
        restore = force_per_head(head.attn)
        hook = head.attn.register_forward_hook(lambda m, i, o: captured.append(o))
        with torch.no_grad():
            head([f.clone() for f in feats])
        hook.remove()
        restore()
        (attn_out, probs), = captured
        assert tuple(probs.shape) == (B, heads, nq, 4) and tuple(attn_out.shape) == (B, nq, E)
        assert probs.dtype == attn_out.dtype == torch.float32
        out[f"{name}/probs"] = probs.numpy()
        out[f"{name}/attn_out"] = attn_out.numpy()
        out[f"{name}/meta"] = np.array([E, heads, nq, B, seed, 1 if pool == "mean" else 0,
                                        1 if ftype.endswith("decoupled") else 0, factor], dtype=np.int64)
        out[f"{name}/qscale"] = np.array([qs if qs is not None else 0.0], dtype=np.float32)
        out[f"{name}/sha"] = np.frombuffer(bytes.fromhex(sha), dtype=np.uint8)
        rows = probs.reshape(-1, 4)
        spread = float(((rows.max(1).values - rows.min(1).values) >= 0.5).float().mean())
        below = float((rows.max(1).values < 0.95).float().mean())
        print(f"head_attn {name}: rows with max - min >= 0.5: {spread:.3f}, rows with peak < 0.95: {below:.3f}")
    path = os.path.join(HERE, "head_attn_golden.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(1)
    main()
