"""The opt-in bf16 matrix-core head on a box without a GPU: its host twin (wv_band_attn_pool_bf16_cpu, csrc/host_head.cpp),
the argument validation of the device entry points and the module-level switch (`head.matrix_dtype`).

Yardstick (tests/golden/head_bf16_golden.npz, made by tests/golden/make_golden_head_bf16.py from the reference's own
module): a bf16 implementation must be no further from the reference's fp32 output than the reference's own bf16 autocast
run is -- rms(y - out32) <= gap_rms, max|y - out32| <= 1.5 gap_max -- and, so that a silent fp32 run cannot pass as bf16,
rms(y - y_fp32_path) >= 0.25 gap_rms.

That yardstick is mostly the bf16 effect itself, so it catches only a gross error.  The sharp one is the numerical contract
(tests/head_contract.py): the twin within 0.25 eff_rms / 1.0 eff_max of the fp64 evaluation of the bf16 oracle, over the shape
sweep of the GPU tests, with features that are NOT bf16-representable."""
import ctypes
import os

import numpy as np
import pytest
import torch

import head_contract as hc
from head_contract import check_gap_bounds as check_bounds, rms
from oracle import head_torch
from wvhash import _lib, synth
from wvhash.models import fusion, get_fusion_head

GOLD = os.path.join(os.path.dirname(__file__), "golden", "head_bf16_golden.npz")
TYPES = {"adv": "cross_attention_advanced", "base": "cross_attention_bottleneck",
         "pooled": "cross_attention_pooled", "decoupled": "cross_attention_decoupled"}
CASES = ["adv_e384_nq4", "adv_e384_nq1", "adv_e384_nq8", "adv_e64_nq4", "base_e384_nq4", "pooled_e384_nq4", "decoupled_e384_nq4"]


def build(n, gold, batch=None, feat_seed=None):
    """Head of golden case n (seeded weights) and bf16-rounded fp32 band features."""
    E, heads, nq, B, seed, mean, dec = gold[n + "/meta"].tolist()
    cfg = {"type": TYPES[n.split("_")[0]], "output_dim": E, "num_heads": heads, "num_queries": nq,
           "sub_band_dropout_p": 0.0, "ortho_weight": 0.1}
    if mean:
        cfg["query_pool"] = "mean"
    qs = float(gold[n + "/qscale"][0])
    if dec:
        cfg["query_scale_init"] = qs
    head = get_fusion_head(cfg, [E] * 4)
    sd = synth.head_state(E, nq, "mean" if mean else "concat", seed, query_scale=qs if dec else None)
    assert bytes.fromhex(synth.state_sha(sd)) == gold[n + "/sha"].tobytes()
    head.load_state_dict(sd)
    feats = synth.band_features(batch or B, E, seed + 1000 if feat_seed is None else feat_seed)
    return head.eval(), [f.bfloat16().float() for f in feats]


def test_fixture_is_complete():
    gold = np.load(GOLD)
    assert sorted({k.split("/")[0] for k in gold.files}) == sorted(CASES)
    for n in CASES:
        E, _, _, B, *_ = gold[n + "/meta"].tolist()
        assert B == 16 and gold[n + "/out32"].shape == (B, E) and gold[n + "/out16"].dtype == np.uint16
        y16 = torch.from_numpy(gold[n + "/out16"].view(np.int16)).view(torch.bfloat16).float()
        d = y16 - torch.from_numpy(gold[n + "/out32"])
        np.testing.assert_allclose([float(d.abs().max()), rms(d)], gold[n + "/gap"], rtol=1e-6)


@pytest.mark.parametrize("n", CASES)
def test_host_twin_sits_inside_the_reference_gap(n):
    gold = np.load(GOLD)
    head, feats = build(n, gold)
    out32 = torch.from_numpy(gold[n + "/out32"])
    args = (head.effective_queries(), head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2], head.out_proj, head._pool == "mean")
    with torch.no_grad():
        y_f32 = fusion.band_attn_pool_host(feats, *args)
        y = fusion.band_attn_pool_host(feats, *args, matrix_dtype="bf16")                                   # fp32-typed features
        y_b = fusion.band_attn_pool_host([f.bfloat16() for f in feats], *args, matrix_dtype=torch.bfloat16)   # bf16-typed
    assert y.dtype == torch.float32 and torch.equal(y, y_b)              # the inputs are bf16-representable: same bits
    assert float((y_f32 - out32).abs().max()) < 5e-5                      # the fp32 twin on these inputs: the fp32 tolerance
    check_bounds(y, y_f32, out32, gold[n + "/gap"], n)


def test_fp32_oracle_residue_leaves_a_margin():
    """The bf16 oracle evaluated in fp32 is itself an fp32 implementation of the contract: its distance from the fp64
    evaluation is what the bounds are sized from.  Every sweep point; the worst ratios are printed and must be the ones
    head_contract's docstring quotes (torch's host GEMM may sum in another order on another machine: then they move a
    little, and the bound itself is what is asserted)."""
    worst_r = worst_m = 0.0
    for config, B in hc.SWEEP:
        ys = hc.yardstick(config, B)
        y = head_torch.band_attn_pool(ys.feats, ys.sd, matrix_dtype="bf16", **ys.kw)
        r, m = ys.check(y, f"fp32 oracle {config} B={B}")
        worst_r, worst_m = max(worst_r, r), max(worst_m, m)
    print(f"fp32 oracle, worst of {len(hc.SWEEP)} points: {worst_r:.3f} x eff_rms, {worst_m:.3f} x eff_max "
          f"(recorded: {hc.FP32_ORACLE_WORST}; bounds {hc.RMS_BOUND}, {hc.MAX_BOUND})")
    assert 2 * hc.FP32_ORACLE_WORST[0] <= hc.RMS_BOUND and 2 * hc.FP32_ORACLE_WORST[1] <= hc.MAX_BOUND


@pytest.mark.parametrize("B", [1, 17, 65])
@pytest.mark.parametrize("config", [c for c in hc.CONFIGS if c != "e384_h8_q8_concat"])
def test_host_twin_meets_the_contract(config, B):
    """fp32-typed features that need rounding; bf16-typed ones (torch's rounding) must give the same bits."""
    ys = hc.yardstick(config, B)
    head = hc.module(config)
    with torch.no_grad():
        y = fusion.band_attn_pool_host(ys.feats, *hc.module_args(head), matrix_dtype="bf16")
        y_b = fusion.band_attn_pool_host([f.bfloat16() for f in ys.feats], *hc.module_args(head), matrix_dtype="bf16")
    assert torch.equal(y, y_b)
    ys.check(y, f"host twin {config} B={B}")


def test_host_twin_rounds_to_nearest_even():
    """Features and weights on and next to bf16 ties of both parities: the twin's own rounding gives the bits that torch's
    rounding of the same values, applied beforehand, gives."""
    config, B = "e96_h8_q5_concat", 17
    E = hc.CONFIGS[config][0]
    feats = [hc.plant(f, 3, 50 + i) for i, f in enumerate(synth.band_features(B, E, seed=77))]
    planted, rounded = hc.planted_state(config)
    with torch.no_grad():
        y = fusion.band_attn_pool_host(feats, *hc.module_args(hc.module(config, planted)), matrix_dtype="bf16")
        y_f = fusion.band_attn_pool_host([f.bfloat16() for f in feats], *hc.module_args(hc.module(config, planted)), matrix_dtype="bf16")
        y_w = fusion.band_attn_pool_host(feats, *hc.module_args(hc.module(config, rounded)), matrix_dtype="bf16")
    assert torch.equal(y, y_f) and torch.equal(y, y_w)
    assert not torch.equal(feats[0], feats[0].bfloat16().float()) and not torch.equal(planted["mlp.0.weight"], rounded["mlp.0.weight"])


def _params(E=384, nq=4):
    p = _lib.HeadParams()
    p.embed_dim, p.num_heads, p.num_queries, p.num_tokens, p.pool_mean = E, 8, nq, 4, 0
    for name, _ in _lib.HeadParams._fields_[5:20]:
        setattr(p, name, 16)                                             # never dereferenced: validation fails first
    p.ln_eps = 1e-5
    return p


def test_argument_validation_happens_on_the_host():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    p = _params()
    big = ctypes.c_size_t(1 << 40)
    assert lib.wv_band_attn_bf16_prepared_bytes(ctypes.byref(p)) == (4 * 384 * 4 + (2 + 1 + 4 + 4 + 4) * 384 * 384 * 2)
    assert lib.wv_band_attn_pool_bf16(ctypes.byref(p), one, one, 7, 8, one, one, big, None) == -22
    assert b"feat_dtype=7" in lib.wv_last_error()
    assert lib.wv_band_attn_pool_bf16(ctypes.byref(p), one, one, _lib.WV_DT_U8, 8, one, one, big, None) == -22
    assert lib.wv_band_attn_pool_bf16(ctypes.byref(p), None, one, _lib.WV_DT_BF16, 8, one, one, big, None) == -22
    assert b"null prepared blob" in lib.wv_last_error()
    assert lib.wv_band_attn_pool_bf16(ctypes.byref(p), one, one, _lib.WV_DT_BF16, 8, one, one, ctypes.c_size_t(64), None) == -12
    assert b"workspace" in lib.wv_last_error()
    assert lib.wv_band_attn_bf16_prepare(ctypes.byref(p), None, None) == -22
    p40 = _params(E=40)
    assert lib.wv_band_attn_bf16_prepared_bytes(ctypes.byref(p40)) == 0      # configuration not covered
    assert lib.wv_band_attn_pool_bf16(ctypes.byref(p40), one, one, _lib.WV_DT_F32, 8, one, one, big, None) == -22
    assert b"embed_dim=40 must be a multiple of 32" in lib.wv_last_error()
    assert lib.wv_band_attn_bf16_prepare(ctypes.byref(p40), one, None) == -22
    assert lib.wv_band_attn_pool_bf16_cpu(ctypes.byref(p40), one, _lib.WV_DT_F32, 8, one) == -22
    assert b"embed_dim=40" in lib.wv_last_error()
    assert lib.wv_band_attn_pool_bf16_cpu(ctypes.byref(p), one, 9, 8, one) == -22 and b"feat_dtype=9" in lib.wv_last_error()
    assert lib.wv_band_attn_pool_bf16_cpu(ctypes.byref(p), None, _lib.WV_DT_F32, 8, one) == -22
    assert lib.wv_band_attn_pool_bf16_workspace_bytes(ctypes.byref(p), 0) == 0
    assert lib.wv_abi_version() == 5                                         # new symbols only


def test_device_entry_point_refuses_what_it_does_not_cover():
    lib = _lib.load()
    p = _params(E=1024, nq=64)
    p.num_tokens = 64
    one = ctypes.c_void_p(16)
    rc = lib.wv_band_attn_pool_bf16(ctypes.byref(p), one, one, _lib.WV_DT_F32, 8, one, one, ctypes.c_size_t(1 << 40), None)
    assert rc == _lib.WV_ENOTSUP and b"LDS" in lib.wv_last_error()


def test_fp32_entry_point_refuses_an_attention_core_that_does_not_fit_the_lds():
    """The plan checks the attention core's LDS for either precision, before any device call: 64 tokens at E = 384, Nq = 4,
    8 heads need (64 x 772 + 4 x 384 + 4 x 8 x 64) x 4 = 211,968 bytes against the CU's 163,840; 4 tokens fit, and the call
    goes on to its next check (the workspace)."""
    lib = _lib.load()
    p = _params()
    one = ctypes.c_void_p(16)
    p.num_tokens = 64
    rc = lib.wv_band_attn_pool(ctypes.byref(p), one, 1, one, one, ctypes.c_size_t(1 << 40), None)
    assert rc == _lib.WV_ENOTSUP and b"LDS" in lib.wv_last_error() and b"band_attn_pool:" in lib.wv_last_error()
    p.num_tokens = 4
    assert lib.wv_band_attn_pool(ctypes.byref(p), one, 1, one, one, ctypes.c_size_t(64), None) == -12
    assert b"workspace" in lib.wv_last_error()


def test_module_switch_on_host_tensors():
    gold = np.load(GOLD)
    head, feats = build("adv_e384_nq4", gold)
    assert head.matrix_dtype is None
    args = (head.effective_queries(), head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2], head.out_proj, False)
    head.host_twin = True
    with torch.no_grad():
        base = fusion.band_attn_pool_host(feats, *args)
        assert torch.equal(head(feats), base)                                # matrix_dtype=None: today's path, bit for bit
        assert torch.equal(fusion.band_attn_pool_host(feats, *args, matrix_dtype=None), base)
        want = fusion.band_attn_pool_host(feats, *args, matrix_dtype="bf16")
        for value in ("bf16", torch.bfloat16):
            head.matrix_dtype = value
            assert torch.equal(head(feats), want) and not torch.equal(want, base)
        head.matrix_dtype = "auto"
        assert torch.equal(head(feats), base)                                # no autocast: fp32
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert torch.equal(head(feats), want)
        head.matrix_dtype = "fp8"
        with pytest.raises(ValueError, match="matrix_dtype"):
            head(feats)


def test_get_fusion_head_reads_matrix_dtype():
    cfg = {"type": "cross_attention_advanced", "output_dim": 64}
    assert get_fusion_head(dict(cfg), [64] * 4).matrix_dtype is None
    for t in TYPES.values():
        assert get_fusion_head(dict(cfg, type=t, matrix_dtype="bf16"), [64] * 4).matrix_dtype == "bf16"
    assert get_fusion_head(dict(cfg, matrix_dtype="auto"), [64] * 4).matrix_dtype == "auto"
    with pytest.raises(ValueError, match="matrix_dtype"):
        get_fusion_head(dict(cfg, matrix_dtype="fp16"), [64] * 4)
