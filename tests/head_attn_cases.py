"""Shared by the attention-map tests (tests/test_host_head_attn.py, tests/test_gpu_head_attn.py): the cases of
tests/golden/head_attn_golden.npz, their truth and the tolerance.

Truth in every test is stock nn.MultiheadAttention in fp64 on the seeded weights (the reference's `attn` is that class).
Tolerance, per output and per case: the error against that truth may be at most max(4 x e_ref, floor), e_ref being the error
of the reference-made fp32 fixture against the same truth and floor 1e-6 for probabilities, 4e-6 for attn_out.  The factor
4 allows another summation order at a few ulps; it is no measured property of the code under test.  The scores have no
reference-made value: they are held to the fp64 truth at 4 x e_scores32, the error of the same stock computation
(F.multi_head_attention_forward's in-projection, query scaling and bmm) carried out in fp32.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import head_torch
from wvhash import synth
from wvhash.models import get_fusion_head

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROB_FLOOR, OUT_FLOOR = 1e-6, 4e-6
# the seven HEAD_CASES of tests/golden/make_golden.py, and three of them with the query tokens x 4 and x 100
NAMES = ["adv_e384_nq1", "adv_e384_nq4", "adv_e384_nq4_x100", "adv_e384_nq4_x4", "adv_e384_nq8", "adv_e384_nq8_x100",
         "adv_e384_nq8_x4", "adv_e64_nq4", "adv_e64_nq4_x100", "adv_e64_nq4_x4", "base_e384_nq4", "decoupled_e384_nq4",
         "pooled_e384_nq4"]
TYPES = {"adv": "cross_attention_advanced", "base": "cross_attention_bottleneck",
         "pooled": "cross_attention_pooled", "decoupled": "cross_attention_decoupled"}


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "head_attn_golden.npz"))


def case_names():
    return sorted(k.split("/")[0] for k in golden().files if k.endswith("/meta"))


def stock_attention(E, heads, sd, dtype, dropout=0.0):
    """nn.MultiheadAttention holding the attn.* tensors of state_dict sd, in eval mode."""
    mha = nn.MultiheadAttention(E, heads, dropout=dropout, batch_first=True).to(dtype).eval()
    mha.load_state_dict({k[len("attn."):]: v.to(dtype) for k, v in sd.items() if k.startswith("attn.")})
    return mha


def stock_scores(mha, q, kv):
    """What F.multi_head_attention_forward takes the softmax of, [B, H, Nq, S], in the dtype of its arguments."""
    E, H = mha.embed_dim, mha.num_heads
    hd = E // H
    w, b = mha.in_proj_weight, mha.in_proj_bias
    Q, K = F.linear(q, w[:E], b[:E]), F.linear(kv, w[E:2 * E], b[E:2 * E])
    B, Nq, S = q.shape[0], q.shape[1], kv.shape[1]
    Qh = Q.view(B, Nq, H, hd).transpose(1, 2).reshape(B * H, Nq, hd) * math.sqrt(1.0 / float(hd))
    Kh = K.view(B, S, H, hd).transpose(1, 2).reshape(B * H, S, hd)
    return torch.bmm(Qh, Kh.transpose(-2, -1)).view(B, H, Nq, S)


class Case:
    """One fixture case: seeded weights and features, the reference-made outputs and the fp64 truth; never modified."""

    def __init__(self, name):
        g = golden()
        self.name = name
        E, heads, nq, B, seed, mean, dec, factor = g[name + "/meta"].tolist()
        self.E, self.heads, self.nq, self.B, self.factor, self.mean, self.dec = E, heads, nq, B, factor, bool(mean), bool(dec)
        self.qscale = float(g[name + "/qscale"][0])
        sd = synth.head_state(E, nq, "mean" if mean else "concat", seed, query_scale=self.qscale if dec else None)
        assert bytes(g[name + "/sha"]).hex() == synth.state_sha(sd), name       # the weights the fixture was made with
        sd["query_tokens"] = sd["query_tokens"] * float(factor)
        self.sd = sd
        self.feats = synth.band_features(B, E, seed + 1000)
        self.kv = torch.stack(self.feats, dim=1)                                  # [B, 4, E]
        self.ref_probs = torch.from_numpy(g[name + "/probs"])
        self.ref_out = torch.from_numpy(g[name + "/attn_out"])
        q = head_torch.effective_queries(sd, self.dec)                            # [1, Nq, E]
        with torch.no_grad():
            m64 = stock_attention(E, heads, sd, torch.float64)
            q64, kv64 = q.double().expand(B, -1, -1), self.kv.double()
            self.out64, self.probs64 = m64(q64, kv64, kv64, need_weights=True, average_attn_weights=False)
            self.scores64 = stock_scores(m64, q64, kv64)
            s32 = stock_scores(stock_attention(E, heads, sd, torch.float32), q.float().expand(B, -1, -1), self.kv)
        assert (torch.softmax(self.scores64, -1) - self.probs64).abs().max() < 1e-12
        self.e_probs = float((self.ref_probs.double() - self.probs64).abs().max())
        self.e_out = float((self.ref_out.double() - self.out64).abs().max())
        self.e_scores32 = float((s32.double() - self.scores64).abs().max())
        self.tol_probs = max(4 * self.e_probs, PROB_FLOOR)
        self.tol_out = max(4 * self.e_out, OUT_FLOOR)
        self.tol_scores = 4 * self.e_scores32

    def module(self):
        """The product's head of this case (host, eval mode) holding its weights."""
        cfg = {"type": TYPES[self.name.split("_")[0]], "output_dim": self.E, "num_heads": self.heads, "num_queries": self.nq,
               "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
        if self.mean:
            cfg["query_pool"] = "mean"
        if self.dec:
            cfg["query_scale_init"] = self.qscale
        head = get_fusion_head(cfg, [self.E] * 4)
        head.load_state_dict(self.sd)
        return head.eval()

    def check(self, maps, what, per_head=True):
        """maps (an AttnMaps, host tensors) against the truth at the tolerance above; prints every figure before it asserts.
        Returns the ratios err / e_ref of (probs, attn_out) and err / e_scores32, None for an absent output."""
        ratios = []
        for label, got, truth, tol, e_ref in (
                ("probs", maps.weights, self.probs64 if per_head else self.probs64.mean(1), self.tol_probs, self.e_probs),
                ("attn_out", maps.attn_output, self.out64, self.tol_out, self.e_out),
                ("scores", maps.scores, self.scores64, self.tol_scores, self.e_scores32)):
            if got is None:
                ratios.append(None)
                continue
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(truth.shape), (what, label, tuple(got.shape))
            err = float((got.double() - truth).abs().max())
            print(f"{what} {self.name} {label}: err {err:.3e}, e_ref {e_ref:.3e} ({err / e_ref:.2f} x), tol {tol:.3e}")
            assert err <= tol, (what, self.name, label, err, tol)
            ratios.append(err / e_ref)
        if maps.scores is not None and maps.weights is not None and per_head:
            d = float((torch.softmax(maps.scores, -1) - maps.weights).abs().max())
            assert d <= self.tol_probs, (what, self.name, "softmax(scores) vs probs", d)
        return ratios


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def shape_case(E, heads, nq, S, B, seed=77):
    """A shape outside the fixture: (sd, kv [B, S, E], q [1, Nq, E], fp64 probs, attn_out, scores, e_scores32, and the fp32
    stock module's own errors for probs and attn_out, which stand in for e_ref)."""
    sd = synth.head_state(E, nq, "concat", seed)
    g = torch.Generator().manual_seed(seed + 1)
    kv = torch.randn(B, S, E, generator=g)
    q = sd["query_tokens"]
    with torch.no_grad():
        m64, m32 = stock_attention(E, heads, sd, torch.float64), stock_attention(E, heads, sd, torch.float32)
        q64, kv64, q32 = q.double().expand(B, -1, -1), kv.double(), q.expand(B, -1, -1)
        out64, probs64 = m64(q64, kv64, kv64, need_weights=True, average_attn_weights=False)
        out32, probs32 = m32(q32, kv, kv, need_weights=True, average_attn_weights=False)
        scores64 = stock_scores(m64, q64, kv64)
        e_s = float((stock_scores(m32, q32, kv).double() - scores64).abs().max())
    tol = dict(probs=max(4 * float((probs32.double() - probs64).abs().max()), PROB_FLOOR),
               attn_out=max(4 * float((out32.double() - out64).abs().max()), OUT_FLOOR), scores=4 * e_s)
    return dict(sd=sd, kv=kv, q=q, probs=probs64, attn_out=out64, scores=scores64, tol=tol)


def shape_module(E, heads, nq, sd):
    head = get_fusion_head({"type": "cross_attention_advanced", "output_dim": E, "num_heads": heads, "num_queries": nq},
                           [E] * 4)
    head.load_state_dict(sd)
    return head.eval()


# ---- the observers of the reference's studies/measure_attention_collapse.py, restated on our own terms
class Capture:
    def __init__(self):
        self.weights, self.qk, self.outputs = [], [], []

    def pre_hook(self, module, args, kwargs):
        q = kwargs.get("query", args[0] if args else None)
        k = kwargs.get("key", args[1] if len(args) > 1 else None)
        if q is not None and k is not None:
            self.qk.append((q.detach().cpu(), k.detach().cpu()))

    def hook(self, module, inputs, output):
        self.outputs.append(output[0].detach().cpu())
        self.weights.append(output[1].detach().cpu())


def force_per_head(attn):
    """Instance-level forward that forces need_weights=True, average_attn_weights=False; returns the restore callback."""
    original = attn.forward

    def forced(*args, **kwargs):
        kwargs["need_weights"] = True
        kwargs["average_attn_weights"] = False
        return original(*args, **kwargs)

    attn.forward = forced
    return lambda: setattr(attn, "forward", original)


def observe(head, run):
    """run() with the three registrations on head.attn; everything is removed again.  Returns (run's result, Capture)."""
    restore = force_per_head(head.attn)
    cap = Capture()
    handles = [head.attn.register_forward_hook(cap.hook), head.attn.register_forward_pre_hook(cap.pre_hook, with_kwargs=True)]
    try:
        with torch.no_grad():
            result = run()
    finally:
        for h in handles:
            h.remove()
        restore()
    return result, cap


class CallCounter:
    """Counts calls of BandMultiheadAttention.forward (patched on the class, so that no instance looks observed) and of
    _lib.wv_band_attn_maps."""

    def __init__(self, monkeypatch):
        from wvhash import _lib
        from wvhash.models import fusion
        self.attn_calls = self.lib_calls = 0
        attn_forward, lib_maps = fusion.BandMultiheadAttention.forward, _lib.wv_band_attn_maps

        def forward(module, *args, **kwargs):
            self.attn_calls += 1
            return attn_forward(module, *args, **kwargs)

        def maps(*args, **kwargs):
            self.lib_calls += 1
            return lib_maps(*args, **kwargs)

        monkeypatch.setattr(fusion.BandMultiheadAttention, "forward", forward)
        monkeypatch.setattr(_lib, "wv_band_attn_maps", maps)
