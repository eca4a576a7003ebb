"""GPU checks of the opt-in bf16 matrix-core head (csrc/head_bf16.hip, `head.matrix_dtype = "bf16"`).

Yardstick as in tests/test_host_head_bf16.py: the reference module's own bf16 autocast run (tests/golden/head_bf16_golden.npz,
`gap` = [max, rms] of its deviation from its fp32 run).  Per case rms(y - fp32 reference) <= gap_rms, max <= 1.5 gap_max, and
rms(y - the fp32 kernel path) >= 0.25 gap_rms (a silent fp32 run cannot pass as bf16).  Every figure is printed before it
is asserted (run with -s to see them)."""
import ctypes

import numpy as np
import pytest
import torch

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


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


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
    head, feats, _, _ = build(n, gold)
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
    blob32 = head._qproj_cache.get("blob")
    key32 = head._qproj_cache.get("key")
    blob16 = head._bf16_cache["entry"][1]
    assert torch.equal(run(head, feats, "bf16"), y0) and head._bf16_cache["entry"][1] is blob16      # cached
    run(head, feats, None)
    assert head._bf16_cache["entry"][1] is blob16 and head._qproj_cache.get("key") == key32          # alternating rebuilds neither
    with torch.no_grad():
        head.out_proj.weight.mul_(1.5)               # read-out weights: in the bf16 blob, not in the fp32 one
    y1 = run(head, feats, "bf16")
    assert not torch.equal(y1, y0) and head._bf16_cache["entry"][1] is not blob16
    assert head._qproj_cache.get("blob") is blob32 and head._qproj_cache.get("key") == key32          # fp32 blob untouched
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
    assert torch.equal(y, direct) and not head._bf16_cache

