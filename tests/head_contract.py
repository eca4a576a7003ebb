"""Shared by the head tests: the numerical contract of the bf16 matrix-core head as a yardstick, and the shape sweep.

Contract (include/wvhash.h, stated independently by oracle/head_torch.band_attn_pool(matrix_dtype="bf16")): both operands of
the five dense weight products are rounded to bf16 (nearest even, from their fp32 value), nothing else is.  Per case, from
the two oracles only:

    ref     = bf16 oracle evaluated in fp64  (the contract without accumulation error)
    eff     = ref - plain fp64 oracle        (the bf16 effect for these inputs and weights), eff_rms, eff_max
    bound   : rms(y - ref) <= 0.25 eff_rms  and  max|y - ref| <= 1.0 eff_max      for the kernel and for the host twin

Where 0.25 / 1.0 come from: the residue of ANY fp32 implementation of the contract is fp32 summation plus an occasional
activation that lands on the other side of a bf16 rounding boundary.  The same oracle evaluated in fp32 is such an
implementation; on the case list below (every SWEEP point, 50 cases; tests/test_host_head_bf16.py prints the figures) it
stays at or below 0.115 eff_rms (typically 0.02-0.08; the worst is e384_h8_q4_concat at B = 15) and 0.35 eff_max -- see
FP32_ORACLE_WORST; the three BIG_POINTS: 0.073 and 0.28.  Two fp32 evaluations with different summation orders differed by
up to 2.5 x (rms) and 3 x (max) of that residue, hence bounds 2.2 x and 2.9 x above the worst of it; an implementation that
truncates instead of rounding sits at 2-3 eff_rms.  The yardstick is the bf16 effect and not the fp32 oracle's own
residue per case because for small E the residue varies by three orders of magnitude between seeds while the effect is
stable (rms 3.5e-3 ... 4.1e-3).
"""
import functools

import torch

from oracle import head_torch
from wvhash import synth
from wvhash.models import get_fusion_head

RMS_BOUND, MAX_BOUND = 0.25, 1.0
# worst ratios of the fp32-evaluated bf16 oracle over every SWEEP point (measured, printed by
# test_host_head_bf16.py::test_fp32_oracle_residue_leaves_a_margin, which also asserts the 2 x margin to the bounds)
FP32_ORACLE_WORST = (0.115, 0.35)

# (E, heads, Nq, read-out).  Products per call: K|V [4B x 2E, K = E], out-projection [B Nq x E, K = E], mlp.0 [B Nq x 4E,
# K = E], mlp.2 [B Nq x E, K = 4E], read-out [B x E, K = Nq E or E].  The plan (head_plan, csrc/head.hpp) -- gemm_bf16: 128 x 128
# tiles (K step 32) when ceil(M/128) ceil(N/128) >= 256, else 64 x 64 tiles with the 64-wide K step when K (per slice) % 64
# == 0, else the 32-wide one; nk = K steps.  readout_ksplit_bf16: the largest ks in 8, 4, 2 with K % (64 ks) == 0,
# K / ks >= 128 and ceil(B/64) ceil(E/64) ks <= 1024.
CONFIGS = {
    "e32_h4_q3_concat": (32, 4, 3, "concat"),     # K = 32: 32-wide step, nk = 1; N = 32 < 64: column guard, clamped W rows;
                                                  # mlp.2 K = 128: 64-wide, nk = 2; read-out K = 96: 32-wide, nk = 3, no split
    "e96_h8_q5_concat": (96, 8, 5, "concat"),     # K = 96: 32-wide, nk = 3; N = 96 / 192: partial column tile; Nq = 5: d5 = 0;
                                                  # mlp.2 K = 384: 64-wide, nk = 6; read-out K = 480: 32-wide, nk = 15, no split
    "e160_h8_q3_mean": (160, 8, 3, "mean"),       # K = 160: 32-wide, nk = 5; Nq = 3: d5 = 2; mlp.2 K = 640: nk = 10; mean read-out
                                                  # K = 160: 32-wide, nk = 5, no split
    "e64_h4_q4_concat": (64, 4, 4, "concat"),     # K = 64: 64-wide, nk = 1; mlp.2 K = 256: nk = 4; read-out K = 256: 2 slices of 128
    "e384_h8_q1_concat": (384, 8, 1, "concat"),   # rmod = 1; K = 384: 64-wide, nk = 6; read-out K = 384: 2 slices of 192 (nk = 3)
    "e384_h8_q4_concat": (384, 8, 4, "concat"),   # read-out K = 1536: 8 slices of 192 while ceil(B/64) <= 21
    "e384_h12_q8_concat": (384, 12, 8, "concat"),  # 12 heads; read-out K = 3072: 8 slices of 384
    "e384_h8_q7_mean": (384, 8, 7, "mean"),       # Nq = 7: d5 = 5; mean read-out K = 384: 2 slices of 192
    "e384_h8_q8_concat": (384, 8, 8, "concat"),   # only at B = 1400 (BIG_POINTS)
}
EDGE_B = (1, 15, 16, 17, 63, 64, 65, 129)   # rows 4B, B Nq and B on both sides of the 64 and 128 tile edges
# every small point runs 64 x 64 tiles by dispatch (at most 5 x 12 tiles of 128)
SWEEP = ([(c, b) for c in ("e32_h4_q3_concat", "e96_h8_q5_concat", "e160_h8_q3_mean", "e64_h4_q4_concat") for b in EDGE_B]
         # B = 120: the K|V product is 8 x 12 tiles of 64 (XCD remap active: 96 % 8 == 0) with a partial last row tile (480 rows)
         + [("e384_h8_q4_concat", b) for b in EDGE_B + (120,)]
         + [(c, b) for c in ("e384_h8_q1_concat", "e384_h12_q8_concat", "e384_h8_q7_mean") for b in (1, 65, 120)])
BIG_POINTS = [
    # read-out 22 x 6 tiles: 8 slices would be 1056 > 1024 workgroups -> 4 slices of 384; K|V (44 x 6) and mlp.0 (44 x 12) on
    # 128 x 128 tiles with a partial last row tile (5600 rows), out-projection and mlp.2 (44 x 3) on 64 x 64
    ("e384_h8_q4_concat", 1400),
    # read-out 43 x 6 tiles: 4 slices would be 1032 > 1024 -> 2 slices of 768; K|V (85 x 6), out-projection / mlp.2 (85 x 3 =
    # 255: 64 x 64 tiles still) and mlp.0 (85 x 12) -- 10800 rows, partial last row tile of either size
    ("e384_h8_q4_concat", 2700),
    # 128 x 128 tiles by dispatch for K|V (44 x 6 = 264), out-projection, mlp.2 (88 x 3 = 264) and mlp.0 (88 x 12), partial
    # last row tiles (5600 and 11200 rows); read-out K = 3072 in 4 slices of 768
    ("e384_h8_q8_concat", 1400),
]
PIN_B = (17, 65, 129)
PINS = ("tile64", "tile128", "tile64-bk32")
CONFIG_INDEX = {name: i for i, name in enumerate(CONFIGS)}


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def set_pin(diag, pin):
    """Pin a GEMM variant of the bf16 head on the diagnostic build (`diag` fixture); None = dispatch."""
    diag.delenv("WV_HEAD_BF16", raising=False)
    diag.delenv("WV_HEAD_BF16_BK", raising=False)
    if pin:
        diag.setenv("WV_HEAD_BF16", pin.split("-")[0])
        if pin.endswith("bk32"):
            diag.setenv("WV_HEAD_BF16_BK", "32")


def state(config):
    E, _, nq, pool = CONFIGS[config]
    return synth.head_state(E, nq, pool, seed=4100 + CONFIG_INDEX[config])


def module(config, sd=None):
    """The product's head module of a configuration (host, eval mode) holding `sd` (default: state(config))."""
    E, heads, nq, pool = CONFIGS[config]
    cfg = {"type": "cross_attention_pooled" if pool == "mean" else "cross_attention_advanced", "output_dim": E,
           "num_heads": heads, "num_queries": nq, "sub_band_dropout_p": 0.0}
    if pool == "mean":
        cfg["query_pool"] = "mean"
    head = get_fusion_head(cfg, [E] * 4)
    head.load_state_dict(state(config) if sd is None else sd)
    return head.eval()


def module_args(head):
    return (head.effective_queries(), head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2], head.out_proj,
            head._pool == "mean")


class Yardstick:
    """Both fp64 oracles of one set of inputs and weights; never modified after it is made."""

    def __init__(self, feats, sd, heads, pool, normalize_queries=False):
        self.feats, self.sd = feats, sd
        self.kw = dict(num_heads=heads, pool=pool, normalize_queries=normalize_queries)
        self.plain64 = head_torch.band_attn_pool(feats, sd, dtype=torch.float64, **self.kw)
        self.ref = head_torch.band_attn_pool(feats, sd, dtype=torch.float64, matrix_dtype="bf16", **self.kw)
        eff = self.ref - self.plain64
        self.eff_rms, self.eff_max = rms(eff), float(eff.abs().max())

    def ratios(self, y):
        e = y.double() - self.ref
        return rms(e) / self.eff_rms, float(e.abs().max()) / self.eff_max

    def check(self, y, what):
        """The bound of the module docstring; prints both ratios before it asserts."""
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(self.ref.shape) and bool(torch.isfinite(y).all()), what
        r, m = self.ratios(y)
        print(f"{what}: rms {r:.3f} x eff_rms ({self.eff_rms:.2e}), max {m:.3f} x eff_max ({self.eff_max:.2e})")
        assert r <= RMS_BOUND, (what, r)
        assert m <= MAX_BOUND, (what, m)
        return r, m


@functools.lru_cache(maxsize=None)
def yardstick(config, B):
    """Sweep point (config, B): seeded weights, seeded fp32 features that are NOT bf16-representable, both oracles."""
    E, heads, _, pool = CONFIGS[config]
    feats = synth.band_features(B, E, seed=9000 + 37 * CONFIG_INDEX[config] + B)
    return Yardstick(feats, state(config), heads, pool)


def check_gap_bounds(y, y_fp32_path, out32, gap, what):
    """The reference-gap bounds (tests/golden/head_bf16_golden.npz): no further from the reference's fp32 output than its own
    autocast run is -- rms <= gap_rms, max <= 1.5 gap_max -- and rms(y - fp32 path) >= 0.25 gap_rms, so that a silent fp32 run
    cannot pass as bf16.  Prints every figure before it asserts."""
    gmax, grms = float(gap[0]), float(gap[1])
    e = y - out32
    r, m, away = rms(e), float(e.abs().max()), rms(y - y_fp32_path)
    print(f"{what}: rms {r:.5f} = {r / grms:.2f} x gap, max {m:.4f} = {m / gmax:.2f} x gap, from the fp32 path {away / grms:.2f} x gap")
    assert r <= 1.0 * grms, what
    assert m <= 1.5 * gmax, what
    assert away >= 0.25 * grms, what


def tie_values(n, seed):
    """n fp32 values around one in magnitude that sit on and next to bf16 rounding boundaries: exact ties of both parities
    (1 + 2^-8 rounds down to the even 1, 1 + 3 2^-8 up to the even 1 + 2^-6), each scaled by 2^-6 ... 2^3 with both signs, and
    the fp32 neighbours one ulp either side of every tie."""
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])
    base = torch.cat([ties, torch.nextafter(ties, torch.tensor(0.0)), torch.nextafter(ties, torch.tensor(4.0))])
    scaled = torch.cat([s * base * 2.0 ** k for k in range(-6, 4) for s in (1.0, -1.0)])          # 120 distinct values
    g = torch.Generator().manual_seed(seed)
    return scaled[torch.randint(scaled.numel(), (n,), generator=g)]


def plant(t, every, seed, scale=1.0):
    """A copy of t with every `every`-th element (row-major) replaced by scale * tie_values (scale a power of two)."""
    out = t.clone().reshape(-1)
    idx = torch.arange(seed % every, out.numel(), every)
    out[idx] = scale * tie_values(idx.numel(), seed)
    return out.reshape(t.shape)


ROUNDED_WEIGHTS = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.0.weight", "mlp.2.weight", "out_proj.weight")


def planted_state(config, seed=0):
    """state(config) with tie values planted (scaled by 2^-4: the magnitude of the weights) in the five weight matrices the
    contract rounds -- the K | V rows of in_proj_weight only -- plus the same state with those matrices rounded by torch."""
    E = CONFIGS[config][0]
    sd = state(config)
    planted, rounded = dict(sd), dict(sd)
    for i, k in enumerate(ROUNDED_WEIGHTS):
        w = sd[k].clone()
        lo = E if k == "attn.in_proj_weight" else 0                  # the Q rows stay as they are, in both copies
        w[lo:] = plant(w[lo:], 5, seed + i, scale=2.0 ** -4)
        planted[k] = w
        rounded[k] = w.clone()
        rounded[k][lo:] = w[lo:].bfloat16().float()
    return planted, rounded
