"""GPU checks of the opt-in bf16 matrix-core head (csrc/head_bf16.hip, `head.matrix_dtype = "bf16"`).

Yardstick as in tests/test_host_head_bf16.py: the reference module's own bf16 autocast run (tests/golden/head_bf16_golden.npz,
`gap` = [max, rms] of its deviation from its fp32 run).  Per case rms(y - fp32 reference) <= gap_rms, max <= 1.5 gap_max, and
rms(y - the fp32 kernel path) >= 0.25 gap_rms (a silent fp32 run cannot pass as bf16).  Every figure is printed before it
is asserted (run with -s to see them).

That yardstick is mostly the bf16 effect itself and catches only a gross error.  The sharp one is the numerical contract
(tests/head_contract.py: within 0.25 eff_rms / 1.0 eff_max of the fp64 evaluation of the bf16 oracle), held over a shape
sweep that reaches every dispatch decision of gemm_bf16 / readout_ksplit_bf16 (head_plan, csrc/head.hpp), plus properties that hold bit for bit:
a row does not depend on where it sits, the rounding is torch's round to nearest even, the caller's buffers are written only
where the kernels own them, and the three tile variants give the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import head_contract as hc
from oracle import head_torch
from wvhash import _lib, synth
from wvhash.models import MultiDinoHashing, fusion, get_fusion_head
from wvhash.models.vit import tiny_vit

pytestmark = pytest.mark.gpu

TYPES = {"adv": "cross_attention_advanced", "base": "cross_attention_bottleneck",
         "pooled": "cross_attention_pooled", "decoupled": "cross_attention_decoupled"}
CASES = ["adv_e384_nq4", "adv_e384_nq1", "adv_e384_nq8", "adv_e64_nq4", "base_e384_nq4", "pooled_e384_nq4", "decoupled_e384_nq4"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/head_bf16_golden.npz")


def build(n, gold, batch=None, feat_seed=None):
    """Head of golden case n on the GPU, bf16-rounded fp32 band features (host), the state_dict and the oracle's kwargs."""
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
    head.load_state_dict(sd)
    feats = [f.bfloat16().float() for f in synth.band_features(batch or B, E, seed + 1000 if feat_seed is None else feat_seed)]
    okw = dict(num_heads=heads, pool="mean" if mean else "concat", normalize_queries=bool(dec))
    return head.cuda().eval(), feats, sd, okw


rms = hc.rms


def run(head, feats, matrix_dtype, dtype=torch.float32):
    head.matrix_dtype = matrix_dtype
    with torch.no_grad():
        return head([f.cuda().to(dtype) for f in feats]).cpu()


@pytest.mark.parametrize("pin", [None, "tile64", "tile128", "tile64-bk32"])
@pytest.mark.parametrize("n", CASES)
def test_golden_cases_sit_inside_the_reference_gap(n, pin, gold, diag):
    """All seven configurations, fp32- and bf16-typed features, every GEMM variant (the diagnostic build pins the tile with
    WV_HEAD_BF16 and the 32-wide K step of the 64-tile -- otherwise taken only when K is not a multiple of 64 -- with
    WV_HEAD_BF16_BK)."""
    diag.delenv("WV_HEAD_BF16", raising=False)
    diag.delenv("WV_HEAD_BF16_BK", raising=False)
    if pin:
        diag.setenv("WV_HEAD_BF16", pin.split("-")[0])
    if pin and pin.endswith("bk32"):
        diag.setenv("WV_HEAD_BF16_BK", "32")
    head, feats, _, _ = build(n, gold)
    out32 = torch.from_numpy(gold[n + "/out32"])
    gmax, grms = (float(v) for v in gold[n + "/gap"])
    y_f32 = run(head, feats, None)
    assert float((y_f32 - out32).abs().max()) < 5e-5
    y = run(head, feats, "bf16")
    y_b = run(head, feats, torch.bfloat16, torch.bfloat16)
    assert y.dtype == torch.float32 and torch.equal(y, y_b)              # bf16-representable inputs: same bits either way
    e = y - out32
    print(f"{n} [{pin}]: rms {rms(e) / grms:.2f} x gap_rms, max {float(e.abs().max()) / gmax:.2f} x gap_max, "
          f"from the fp32 path {rms(y - y_f32) / grms:.2f} x gap_rms")
    assert rms(e) <= 1.0 * grms and float(e.abs().max()) <= 1.5 * gmax
    assert rms(y - y_f32) >= 0.25 * grms


@pytest.mark.parametrize("n,B", [("adv_e384_nq4", b) for b in (1, 63, 200, 1000, 1155, 2048)] +
                         [("adv_e384_nq8", b) for b in (37, 600, 4096)])
def test_batch_sizes_against_the_fp64_oracle(n, B, gold):
    """Partial last tiles, both tile sizes by dispatch; weights of the matching golden case, so that case's gap applies."""
    head, feats, sd, okw = build(n, gold, batch=B, feat_seed=7000 + B)
    E = feats[0].shape[1]
    gmax, grms = (float(v) for v in gold[n + "/gap"])
    ref = head_torch.band_attn_pool(feats, sd, dtype=torch.float64, **okw).float()
    y = run(head, feats, "bf16")
    y2 = run(head, feats, "bf16")
    yb = run(head, feats, "bf16", torch.bfloat16)
    assert torch.equal(y, y2) and torch.equal(y, yb)                     # deterministic; feature dtype does not matter
    e = y - ref
    print(f"{n} B={B}: rms {rms(e) / grms:.2f} x gap_rms, max {float(e.abs().max()) / gmax:.2f} x gap_max")
    assert float(e.abs().max()) <= 1.5 * gmax
    if B * E >= 6144:
        assert rms(e) <= 1.0 * grms


@pytest.mark.parametrize("n", CASES)
def test_kernel_and_host_twin_are_closer_to_each_other_than_to_fp32(n, gold):
    """... and each of them is within the contract's bound of the fp64 evaluation of the bf16 oracle."""
    head, feats, sd, okw = build(n, gold)
    out32 = torch.from_numpy(gold[n + "/out32"])
    y = run(head, feats, "bf16")
    cpu_head = build(n, gold)[0].cpu()
    args = (cpu_head.effective_queries(), cpu_head.attn, cpu_head.norm1, cpu_head.norm2, cpu_head.mlp[0], cpu_head.mlp[2],
            cpu_head.out_proj, cpu_head._pool == "mean")
    with torch.no_grad():
        twin = fusion.band_attn_pool_host(feats, *args, matrix_dtype="bf16")
    d, far = y - twin, y - out32
    print(f"{n}: kernel vs host twin rms {rms(d):.2e} max {float(d.abs().max()):.2e}; kernel vs out32 rms {rms(far):.2e} "
          f"max {float(far.abs().max()):.2e}")
    assert rms(d) < rms(far) and float(d.abs().max()) < float(far.abs().max())
    ys = hc.Yardstick(feats, sd, okw["num_heads"], okw["pool"], okw["normalize_queries"])
    ys.check(y, f"{n}: kernel")
    ys.check(twin, f"{n}: host twin")


def test_bf16_features_are_consumed_in_place(gold):
    head, feats, _, _ = build("adv_e384_nq4", gold, batch=1024)
    head.matrix_dtype = "bf16"
    buf = torch.stack(feats).cuda().bfloat16().contiguous()             # [4, B, E], as a backbone would have written it
    bands = list(buf.unbind(0))
    st = fusion._stacked(bands, keep_bf16=True)
    assert st.dtype == torch.bfloat16 and st.data_ptr() == buf.data_ptr() and tuple(st.shape) == tuple(buf.shape)
    with torch.no_grad():
        want = head(bands)                                              # warm: blob made, allocator pools filled
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        got = head(bands)
        torch.cuda.synchronize()
        delta = torch.cuda.memory_allocated() - before
    print(f"memory_allocated delta {delta} bytes; one fp32 copy of the features is {buf.numel() * 4}")
    assert torch.equal(got, want) and delta < buf.numel() * 4
    # separate bf16 tensors are stacked in their own dtype, never upcast
    st2 = fusion._stacked([b.clone() for b in bands], keep_bf16=True)
    assert st2.dtype == torch.bfloat16 and torch.equal(st2, buf)
    assert fusion._stacked(bands).dtype == torch.float32                 # the fp32 head still gets fp32


def test_auto_follows_autocast_and_the_c4_model_runs_end_to_end(gold):
    head, feats, _, _ = build("adv_e384_nq8", gold)
    y_f32 = run(head, feats, None)
    y_b = run(head, feats, "bf16")
    assert torch.equal(run(head, feats, "auto"), y_f32)                  # outside autocast: the fp32 head
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(run(head, feats, "auto"), y_b)
        assert torch.equal(run(head, feats, None), y_f32)                # opt-in: None stays fp32 under autocast too
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(run(head, feats, "auto"), y_f32)
    # BASELINE c4: one backbone per sub-band, 8 queries, 128 bits
    torch.manual_seed(0)
    cfg = {"type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "num_queries": 8, "sub_band_dropout_p": 0,
           "ortho_weight": 0.1, "dropout": 0.1}
    net = MultiDinoHashing([{"name": "dinov2_vits14"}] * 4, cfg, {"nbits": 128}, backbones=[tiny_vit() for _ in range(4)]).cuda().eval()
    net.set_wavelet(level=1, wavelet="haar")
    img = torch.from_numpy(synth.natural_images(64, 224, 224, seed=3)).permute(0, 3, 1, 2).contiguous().cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        codes32 = net(img)
        net.fusion_head.matrix_dtype = "auto"
        codes16 = net(img)
    assert tuple(codes16.shape) == (64, 128) and set(codes16.unique().tolist()) <= {-1.0, 1.0}
    print(f"c4 shape: {float((codes16 != codes32).float().mean()) * 100:.2f} % of the bits differ from the fp32 head")


def test_parameter_update_invalidates_the_bf16_blob_only(gold):
    head, feats, _, _ = build("adv_e384_nq4", gold)
    y0_f32, y0 = run(head, feats, None), run(head, feats, "bf16")
    peek = lambda slot: head._prepared.peek(slot, head.query_tokens.device)        # noqa: E731   (key, Prepared(blob, qp))
    key32, blob32 = peek("fp32")[0], peek("fp32")[1].blob
    blob16 = peek("bf16")[1].blob
    assert blob32 is not None and blob16 is not None
    assert torch.equal(run(head, feats, "bf16"), y0) and peek("bf16")[1].blob is blob16              # cached
    run(head, feats, None)
    assert peek("bf16")[1].blob is blob16 and peek("fp32")[0] == key32                                # alternating rebuilds neither
    with torch.no_grad():
        head.out_proj.weight.mul_(1.5)               # read-out weights: in the bf16 blob, not in the fp32 one
    y1 = run(head, feats, "bf16")
    assert not torch.equal(y1, y0) and peek("bf16")[1].blob is not blob16
    assert peek("fp32")[1].blob is blob32 and peek("fp32")[0] == key32                                # fp32 blob untouched
    y1_f32 = run(head, feats, None)
    assert not torch.equal(y1_f32, y0_f32)           # (the fp32 path reads out_proj from the parameters)
    with torch.no_grad():
        head.mlp[0].weight.mul_(0.5)
    assert not torch.equal(run(head, feats, "bf16"), y1)


def test_default_is_the_existing_fp32_entry_point(gold):
    head, feats, _, _ = build("adv_e384_nq4", gold)
    assert head.matrix_dtype is None
    dev = [f.cuda() for f in feats]
    with torch.no_grad():
        y = head(dev)
        direct = fusion.band_attn_pool(dev, head.effective_queries(), head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2],
                                       head.out_proj, False)
    assert torch.equal(y, direct) and head._prepared.peek("bf16", y.device) is None



# ---- the numerical contract over the shape sweep (tests/head_contract.py) -------------------------------------------------

@functools.lru_cache(maxsize=None)
def gpu_head(config):
    """One module per configuration for the tests that only run it (its prepared bf16 blob is made once)."""
    return hc.module(config).cuda()


@pytest.mark.parametrize("config,B", hc.SWEEP + hc.BIG_POINTS, ids=lambda v: str(v))
def test_sweep_meets_the_contract_by_dispatch(config, B):
    """Every sweep point as callers get it (release library, dispatch as worked out in head_contract.CONFIGS / SWEEP /
    BIG_POINTS); fp32 features that are not bf16-representable."""
    ys = hc.yardstick(config, B)
    ys.check(run(gpu_head(config), ys.feats, "bf16"), f"kernel {config} B={B}")


@pytest.mark.parametrize("pin", hc.PINS)
@pytest.mark.parametrize("config,B", [(c, b) for c in hc.CONFIGS if c != "e384_h8_q8_concat" for b in hc.PIN_B], ids=lambda v: str(v))
def test_sweep_meets_the_contract_under_every_tile_variant(config, B, pin, diag):
    """tile128 (K step 32) and the 32-wide K step of the 64-tile are otherwise reached only by large batches / K % 64 != 0."""
    hc.set_pin(diag, pin)
    ys = hc.yardstick(config, B)
    ys.check(run(gpu_head(config), ys.feats, "bf16"), f"kernel [{pin}] {config} B={B}")


@pytest.mark.parametrize("pin", (None,) + hc.PINS)
@pytest.mark.parametrize("config,B", [("e96_h8_q5_concat", 65), ("e384_h8_q4_concat", 65), ("e384_h8_q4_concat", 120)], ids=lambda v: str(v))
def test_a_row_does_not_depend_on_its_position(config, B, pin, diag):
    """Same B, same dispatch: permuting the samples permutes the output rows bit for bit (every output element is a function
    of its own sample only) -- whatever tile, wave, lane or split-K slice the sample lands in."""
    hc.set_pin(diag, pin)
    ys = hc.yardstick(config, B)
    head = gpu_head(config)
    y = run(head, ys.feats, "bf16")
    ys.check(y, f"kernel [{pin}] {config} B={B}")
    perms = {"reversed": torch.arange(B - 1, -1, -1), "shuffled": torch.randperm(B, generator=torch.Generator().manual_seed(B))}
    for name, perm in perms.items():
        yp = run(head, [f[perm].contiguous() for f in ys.feats], "bf16")
        bad = (yp != y[perm]).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"{name}: rows {bad[:8]} of the permuted batch differ"


@pytest.mark.parametrize("config,B", [("e96_h8_q5_concat", 65), ("e384_h8_q4_concat", 65)], ids=lambda v: str(v))
def test_operands_are_rounded_to_nearest_even_where_the_contract_says(config, B):
    """Features and weights full of bf16 ties of both parities and of their fp32 neighbours (head_contract.tie_values).
    Features: fp32-typed ones (rounded by Raw8<float>::packed on their way to LDS) give the bits of torch's feats.bfloat16()
    passed as bf16 tensors.  Weights: a module that holds the planted fp32 matrices (rounded by k_to_bf16) gives the bits of
    a module that holds their torch-rounded copies.  The Q rows of in_proj_weight and the biases are not planted: they are
    not rounded, and equal in both modules."""
    E = hc.CONFIGS[config][0]
    feats = [hc.plant(f, 3, 50 + i) for i, f in enumerate(synth.band_features(B, E, seed=77))]
    planted, rounded = hc.planted_state(config)
    assert not torch.equal(feats[0], feats[0].bfloat16().float())
    assert all(not torch.equal(planted[k], rounded[k]) for k in hc.ROUNDED_WEIGHTS)
    assert torch.equal(planted["attn.in_proj_weight"][:E], rounded["attn.in_proj_weight"][:E])
    head = hc.module(config, planted).cuda()
    y = run(head, feats, "bf16")
    y_f = run(head, [f.bfloat16() for f in feats], "bf16", torch.bfloat16)
    assert torch.equal(y, y_f), "fp32-typed features are not rounded as torch rounds them"
    y_w = run(hc.module(config, rounded).cuda(), feats, "bf16")
    assert torch.equal(y, y_w), "the prepared weights are not torch's round-to-nearest-even copies"
    hc.Yardstick(feats, planted, hc.CONFIGS[config][1], hc.CONFIGS[config][3]).check(y, f"planted ties {config} B={B}")


def c_params(head, S=4):
    """wv_head_params of a CUDA module (as fusion.band_attn_pool fills it) and the tensors that keep its pointers alive."""
    E = head.norm1.normalized_shape[0]
    keep = [t.detach().float().contiguous() for t in
            (head.effective_queries().reshape(-1, E), head.attn.in_proj_weight, head.attn.in_proj_bias, head.attn.out_proj.weight,
             head.attn.out_proj.bias, head.norm1.weight, head.norm1.bias, head.mlp[0].weight, head.mlp[0].bias, head.mlp[2].weight,
             head.mlp[2].bias, head.out_proj.weight, head.out_proj.bias, head.norm2.weight, head.norm2.bias)]
    p = _lib.HeadParams()
    p.embed_dim, p.num_heads, p.num_queries, p.num_tokens = E, head.attn.num_heads, keep[0].shape[0], S
    p.pool_mean = 1 if head._pool == "mean" else 0
    (p.q_eff, p.in_proj_w, p.in_proj_b, p.attn_out_w, p.attn_out_b, p.norm1_w, p.norm1_b, p.mlp0_w, p.mlp0_b,
     p.mlp2_w, p.mlp2_b, p.out_w, p.out_b, p.norm2_w, p.norm2_b) = [t.data_ptr() for t in keep]
    p.ln_eps = float(head.norm1.eps)
    p.q_proj = None
    p.prepared = None
    return p, keep


@pytest.mark.parametrize("config,B", [("e384_h8_q4_concat", 65), ("e160_h8_q3_mean", 17)], ids=lambda v: str(v))
def test_the_callers_buffers_are_written_only_where_they_are_owned(config, B):
    """A caller-made workspace of exactly the advertised size plus a 4 KiB tail, and an output buffer with 8 rows to spare:
    tail and spare rows keep their fill, and the result does not depend on what the workspace held before (zeros or an
    all-ones bit pattern, NaN as fp32 and as bf16) -- nothing is read that was not written, split-K partials included
    (8 slices at E = 384, Nq = 4)."""
    lib = _lib.require_gpu()
    ys = hc.yardstick(config, B)
    head = gpu_head(config)
    E = hc.CONFIGS[config][0]
    dev = [f.cuda() for f in ys.feats]
    p, keep = c_params(head)
    need = lib.wv_band_attn_pool_bf16_workspace_bytes(ctypes.byref(p), B)
    assert need > 0
    TAIL, FILL = 4096, 0xA5
    outs = {}
    for name, byte in (("zeros", 0x00), ("nan", 0xFF)):
        ws = torch.full((need + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        ws[:need] = byte
        with torch.no_grad():
            outs[name] = fusion.band_attn_pool(dev, *hc.module_args(head), workspace=ws, matrix_dtype="bf16").cpu()
        assert bool((ws[need:] == FILL).all()), f"{name}: bytes past the advertised workspace size were written"
    ys.check(outs["zeros"], f"caller workspace {config} B={B}")
    assert torch.equal(outs["zeros"], outs["nan"]), "the result depends on what the workspace held before the call"
    assert torch.equal(outs["zeros"], run(head, ys.feats, "bf16"))
    # through the C ABI: the workspace at exactly its advertised size, the output rows B ... B + 7 are not the call's
    blob = torch.empty(lib.wv_band_attn_bf16_prepared_bytes(ctypes.byref(p)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.wv_band_attn_bf16_prepare(ctypes.byref(p), _lib.ptr(blob), _lib.stream_ptr()), "wv_band_attn_bf16_prepare")
    feats = torch.stack(dev).contiguous()
    ws = torch.full((need + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((B + 8, E), -7777.0, device="cuda")
    rc = lib.wv_band_attn_pool_bf16(ctypes.byref(p), _lib.ptr(blob), _lib.ptr(feats), _lib.WV_DT_F32, B, _lib.ptr(out), _lib.ptr(ws),
                                    ctypes.c_size_t(need), _lib.stream_ptr())
    _lib.check(rc, "wv_band_attn_pool_bf16")
    torch.cuda.synchronize()
    assert bool((out[B:] == -7777.0).all()), "rows past B of the output buffer were written"
    assert bool((ws[need:] == FILL).all())
    assert torch.equal(out[:B].cpu(), outs["zeros"])
    del keep


def test_tile_variants_walk_k_in_the_same_order(diag):
    """64 x 64 tiles with the 64-wide and the 32-wide K step and 128 x 128 tiles all feed k upwards through the same
    v_mfma_f32_32x32x16_bf16 in 16-wide steps, and an output element's accumulator sees nothing else: the same bits."""
    outs = {}
    for config, B in (("e384_h8_q4_concat", 129), ("e96_h8_q5_concat", 65)):
        ys = hc.yardstick(config, B)
        for pin in hc.PINS:
            hc.set_pin(diag, pin)
            outs[pin] = run(gpu_head(config), ys.feats, "bf16")
            ys.check(outs[pin], f"kernel [{pin}] {config} B={B}")
        for pin in hc.PINS[1:]:
            d = outs[pin] - outs[hc.PINS[0]]
            same = torch.equal(outs[pin], outs[hc.PINS[0]])
            print(f"{config} B={B}: {pin} vs {hc.PINS[0]}: {'equal' if same else 'DIFFERENT'}, max |d| {float(d.abs().max()):.2e}")
            assert same, (config, B, pin)                         # measured on MI355X: equal
