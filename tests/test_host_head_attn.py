"""The attention maps of the band-attention head on the host: wv_band_attn_maps_cpu (csrc/host_head.cpp) against the
reference-made fixture tests/golden/head_attn_golden.npz and the fp64 truth (tests/head_attn_cases.py: truth, tolerance),
the argument rules of both entry points (answered on the host, so the GPU one is asked here too), and heads whose `attn`
submodule is observed the way the reference's attention.py and studies/measure_attention_collapse.py observe it.

Measured here, error over e_ref (the fixture's own error against the fp64 truth) over the 13 cases and both layouts:
probs 0.29 - 1.63 x (factor 4: 0.29 - 0.50, factor 100: 0.33 - 0.42), attn_out 0.25 - 1.32 x (factor 4: 0.35 - 0.41, factor 100:
0.43 - 0.51); scores 0.46 - 0.93 x e_scores32.  The bound is 4 x."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import head_attn_cases as hac
from wvhash import _lib
from wvhash.models import SharedDinoHashing, fusion
from wvhash.models.vit import tiny_vit

NAMES = hac.NAMES


def test_fixture_holds_the_thirteen_cases_and_informative_attention():
    """The seven HEAD_CASES and three of them with the query tokens x 4 and x 100.  Over the factor-4 cases at least 70 % of
    the softmax rows spread by 0.5 or more and at least 90 % peak below 0.95: attention that is neither uniform nor one-hot
    (per case at B = 6: spread 0.72 - 0.77, peak 0.89 - 0.93; the rows of the three cases are counted together).  Factor 100
    has scores beyond +-88, where expf overflows without the max subtraction."""
    assert hac.case_names() == NAMES
    g = hac.golden()
    rows = torch.cat([torch.from_numpy(g[n + "/probs"]).reshape(-1, 4) for n in NAMES if n.endswith("_x4")])
    for n in NAMES:
        c = hac.case(n)
        assert c.ref_probs.shape == (c.B, c.heads, c.nq, 4) and c.ref_out.shape == (c.B, c.nq, c.E)
        assert c.B == 6 or c.factor == 1
        if c.factor == 100:
            assert float(c.scores64.abs().max()) > 100
    spread = float(((rows.max(1).values - rows.min(1).values) >= 0.5).float().mean())
    below = float((rows.max(1).values < 0.95).float().mean())
    print(f"factor 4: {rows.shape[0]} rows, spread >= 0.5: {spread:.3f}, peak < 0.95: {below:.3f}")
    assert spread >= 0.7 and below >= 0.9


@pytest.mark.parametrize("layout", ["bse", "sbe"])
@pytest.mark.parametrize("name", NAMES)
def test_twin_against_fixture_and_truth(name, layout):
    c = hac.case(name)
    head = c.module()
    kv = c.kv if layout == "bse" else c.kv.transpose(0, 1).contiguous()
    maps = fusion.band_attn_maps(kv, head.effective_queries(), head.attn, layout)
    c.check(maps, f"twin/{layout}")
    sums = maps.weights.double().sum(-1)
    assert float((sums - 1).abs().max()) <= 4e-7 * 4                      # rows sum to 1 within 4e-7 S
    mean = fusion.band_attn_maps(kv, head.effective_queries(), head.attn, layout, per_head=False, want=("probs",))
    assert mean.scores is None and mean.attn_output is None
    c.check(mean, f"twin/{layout}/mean", per_head=False)


def test_twin_probs_mean_against_the_head_fixture(golden_dir):
    """The head-averaged weights the reference's module returned by default, already in head_golden.npz (attn_w)."""
    gold = np.load(f"{golden_dir}/head_golden.npz")
    for name in NAMES:
        c = hac.case(name)
        if c.factor != 1:
            continue
        ref = torch.from_numpy(gold[name + "/attn_w"])
        head = c.module()
        got = fusion.band_attn_maps(c.kv, head.effective_queries(), head.attn, per_head=False, want=("probs",)).weights
        truth = c.probs64.mean(1)
        e_ref, err = float((ref.double() - truth).abs().max()), float((got.double() - truth).abs().max())
        print(f"{name} probs_mean: err {err:.3e}, e_ref {e_ref:.3e}")
        assert got.shape == ref.shape and err <= max(4 * e_ref, hac.PROB_FLOOR)


def raw_params(c, head):
    keep = [t.detach().float().contiguous() for t in (head.effective_queries().reshape(-1, c.E), head.attn.in_proj_weight,
                                                      head.attn.in_proj_bias, head.attn.out_proj.weight, head.attn.out_proj.bias)]
    p = _lib.HeadParams()
    p.embed_dim, p.num_heads, p.num_queries, p.num_tokens = c.E, c.heads, c.nq, 4
    p.q_eff, p.in_proj_w, p.in_proj_b, p.attn_out_w, p.attn_out_b = [t.data_ptr() for t in keep]
    return p, keep


def test_every_subset_of_outputs_gives_the_same_values():
    c = hac.case("adv_e64_nq4_x4")
    head = c.module()
    p, keep = raw_params(c, head)
    lib = _lib.load()
    shapes = [(c.B, c.heads, c.nq, 4), (c.B, c.nq, 4), (c.B, c.heads, c.nq, 4), (c.B, c.nq, c.E)]
    full = [torch.full(s, 7.0) for s in shapes]
    assert lib.wv_band_attn_maps_cpu(ctypes.byref(p), _lib.ptr(c.kv), _lib.WV_TOKENS_BSE, c.B, *[_lib.ptr(t) for t in full]) == 0
    for mask in itertools.product((False, True), repeat=4):
        outs = [torch.full(s, 7.0) if on else None for s, on in zip(shapes, mask)]
        rc = lib.wv_band_attn_maps_cpu(ctypes.byref(p), _lib.ptr(c.kv), _lib.WV_TOKENS_BSE, c.B, *[_lib.ptr(t) for t in outs])
        if not any(mask):
            assert rc == -22 and b"no output" in lib.wv_last_error()
            continue
        assert rc == 0
        for got, want in zip(outs, full):
            assert got is None or torch.equal(got, want), mask


def test_refusals_of_both_entry_points():
    c = hac.case("adv_e64_nq4")
    head = c.module()
    p, keep = raw_params(c, head)
    lib = _lib.load()
    one = ctypes.c_void_p(16)                   # never dereferenced: every refusal is answered first
    out = torch.full((c.B, c.heads, c.nq, 4), 7.0)
    big = ctypes.c_size_t(1 << 30)

    def cpu(pp, layout, B, *outs):
        return lib.wv_band_attn_maps_cpu(ctypes.byref(pp), _lib.ptr(c.kv), layout, B, *outs)

    def gpu(pp, layout, B, *outs, ws=one, nbytes=big):
        return lib.wv_band_attn_maps(ctypes.byref(pp), one, layout, B, *outs, ws, nbytes, None)

    for call, o in ((cpu, _lib.ptr(out)), (gpu, one)):
        assert call(p, 1, 0, o, None, None, None) == 0                                  # B == 0: nothing to do ...
        assert bool((out == 7.0).all())                                                 # ... and nothing touched
        assert call(p, 1, c.B, None, None, None, None) == -22 and b"no output" in lib.wv_last_error()
        assert call(p, 2, c.B, o, None, None, None) == -22 and b"layout=2" in lib.wv_last_error()
        assert call(p, -1, c.B, o, None, None, None) == -22
        assert call(p, 1, -1, o, None, None, None) == -22 and b"B=-1" in lib.wv_last_error()
        for field, value, text in (("num_tokens", 65, b"num_tokens=65"), ("num_tokens", 0, b"num_tokens=0"),
                                   ("num_queries", 65, b"num_queries=65"), ("num_heads", 7, b"not divisible"),
                                   ("embed_dim", 60, b"multiple of 8"), ("in_proj_b", None, b"null weight")):
            q = _lib.HeadParams.from_buffer_copy(p)
            setattr(q, field, value)
            assert call(q, 1, c.B, o, None, None, None) == -22 and text in lib.wv_last_error(), field
    # only the attention part of the parameters is read: the pointers of the MLP, the norms and the read-out are NULL here
    assert p.norm1_w is None and p.out_w is None and cpu(p, 1, c.B, _lib.ptr(out), None, None, None) == 0
    # the kernel's LDS: the sentence of wv_band_attn_pool's refusal
    q = _lib.HeadParams.from_buffer_copy(p)
    q.embed_dim, q.num_tokens = 384, 64
    assert gpu(q, 1, 2, one, None, None, None) == _lib.WV_ENOTSUP
    assert b"band_attn_maps: 64 tokens x 4 queries at embed_dim=384 do not fit the attention kernel's LDS" in lib.wv_last_error()
    # a short workspace is refused with the need in the text
    need = lib.wv_band_attn_maps_workspace_bytes(ctypes.byref(p), c.B)
    assert need >= 4 * (c.nq * c.E + 4 * c.B * 2 * c.E + c.B * c.nq * c.E)
    assert gpu(p, 1, c.B, one, None, None, None, nbytes=ctypes.c_size_t(need - 1)) == -22
    assert f"{need - 1} < {need} bytes".encode() in lib.wv_last_error()
    assert gpu(p, 1, c.B, one, None, None, None, ws=None) == -22
    with pytest.raises(ValueError):
        fusion.band_attn_maps(c.kv, head.effective_queries(), head.attn, "esb")
    with pytest.raises(ValueError):
        fusion.band_attn_maps(c.kv, head.effective_queries(), head.attn, want=())


def test_bf16_tokens_are_upcast():
    c = hac.case("adv_e64_nq4")
    head = c.module()
    kv16 = c.kv.bfloat16()
    a = fusion.band_attn_maps(kv16, head.effective_queries(), head.attn)
    b = fusion.band_attn_maps(kv16.float(), head.effective_queries(), head.attn)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["adv_e384_nq4_x4", "base_e384_nq4", "pooled_e384_nq4", "decoupled_e384_nq4", "adv_e64_nq4"])
def test_observed_host_head(name, monkeypatch):
    """studies/measure_attention_collapse.py's three registrations on a host-twin head in eval mode: per-head weights and the
    (query, key) the module was called with arrive, the head's output keeps its bits, and once they are gone `attn` is no
    longer called."""
    c = hac.case(name)
    head = c.module()
    head.host_twin = True
    counter = hac.CallCounter(monkeypatch)
    with torch.no_grad():
        plain = head(c.feats)
    assert counter.attn_calls == 0 and counter.lib_calls == 0                  # unobserved: today's forward
    observed, cap = hac.observe(head, lambda: head(c.feats))
    assert torch.equal(plain, observed)
    assert counter.attn_calls == 1 and counter.lib_calls == 1
    (w,), (out,), ((q, k),) = cap.weights, cap.outputs, cap.qk
    assert tuple(w.shape) == (c.B, 8, c.nq, 4) and tuple(out.shape) == (c.B, c.nq, c.E)
    assert tuple(q.shape) == (c.B, c.nq, c.E) and torch.equal(k, c.kv)
    assert torch.equal(q[0], head.effective_queries()[0].detach()) and torch.equal(q[-1], q[0])
    c.check(fusion.AttnMaps(w, None, out), "observed host head")
    with torch.no_grad():
        again = head(c.feats)
    assert torch.equal(plain, again) and counter.attn_calls == 1 and counter.lib_calls == 1
    assert not head._attn_observed()


def test_plain_forward_hook_receives_averaged_weights():
    """attention.py's hook: output[1] of the default call is the mean over the heads, [B, Nq, 4]."""
    c = hac.case("adv_e384_nq4_x4")
    head = c.module()
    head.host_twin = True
    got = []
    handle = head.attn.register_forward_hook(lambda module, inputs, output: got.append(output[1]))
    with torch.no_grad():
        head(c.feats)
    handle.remove()
    (w,) = got
    assert tuple(w.shape) == (c.B, c.nq, 4)
    c.check(fusion.AttnMaps(w, None, None), "plain hook", per_head=False)
    maps = head.attention_maps(c.feats)
    assert torch.equal(maps, w)
    per_head, scores = head.attention_maps(c.feats, per_head=True, scores=True)
    c.check(fusion.AttnMaps(per_head, scores, None), "attention_maps")


def test_attn_module_keeps_the_stock_surface():
    """Same class family, parameters and state_dict keys; every call the library path does not cover is stock PyTorch."""
    c = hac.case("adv_e64_nq4")
    head = c.module()
    stock = hac.stock_attention(c.E, c.heads, c.sd, torch.float32, dropout=head.attn.dropout)
    assert isinstance(head.attn, torch.nn.MultiheadAttention)
    assert list(head.attn.state_dict()) == list(stock.state_dict())
    q = head.effective_queries().detach().expand(c.B, -1, -1)
    with torch.no_grad():
        per_sample = q.contiguous()                                              # not a broadcast: stock
        a, b = head.attn(per_sample, c.kv, c.kv), stock(per_sample, c.kv, c.kv)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        mask = torch.zeros(c.B, 4, dtype=torch.bool)                             # a mask: stock
        a, b = head.attn(q, c.kv, c.kv, key_padding_mask=mask), stock(q, c.kv, c.kv, key_padding_mask=mask)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        out, w = head.attn(q, c.kv, c.kv, need_weights=False)                    # the library path
        assert w is None and tuple(out.shape) == (c.B, c.nq, c.E)
    head.train()
    torch.manual_seed(0)
    a = head.attn(q, c.kv, c.kv)
    torch.manual_seed(0)
    b = stock.train()(q, c.kv, c.kv)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].requires_grad


def test_collapse_study_sequence_on_a_whole_model(monkeypatch):
    """The statements of the reference's run_diagnostic, from forcing per-head weights to the torch.cat of what was captured,
    on our own model and data: [N, heads, Nq, 4] with rows summing to 1, and the codes keep their bits."""
    torch.manual_seed(5)
    fusion_cfg = {"type": "cross_attention_advanced", "output_dim": 384, "num_queries": 4, "num_heads": 8}
    net = SharedDinoHashing({"name": "dinov2_vits14", "frozen": True}, fusion_cfg, {"nbits": 32},
                            backbone=tiny_vit(384, 28)).eval()
    net.hash_fc.weight.data.mul_(50)
    for pname, prm in net.named_parameters():                                    # LayerScale starts at 1e-5: let the CLS token
        if pname.endswith(".gamma"):                                             # depend on the band
            prm.data.fill_(1.0)
    net.fusion_head.query_tokens.data.mul_(200)                                  # trunc_normal(std 0.02) -> attention that moves
    net.host_twin = net.fusion_head.host_twin = True
    batches = [torch.randn(3, 3, 4, 28, 28) for _ in range(2)]
    with torch.no_grad():
        plain = [net(x) for x in batches]

    fusion_head = net.fusion_head
    restore_attn = hac.force_per_head(fusion_head.attn)
    capture = hac.Capture()
    handles = [fusion_head.attn.register_forward_hook(capture.hook),
               fusion_head.attn.register_forward_pre_hook(capture.pre_hook, with_kwargs=True)]
    band_embeds = []
    for proj in fusion_head.projections:
        handles.append(proj.register_forward_hook(lambda module, inputs, output: band_embeds.append(output.detach())))
    with torch.no_grad():
        observed = [net(x) for x in batches]
    for h in handles:
        h.remove()
    restore_attn()
    all_attn_per_head = torch.cat(capture.weights, dim=0)

    assert tuple(all_attn_per_head.shape) == (6, 8, 4, 4)
    assert float((all_attn_per_head.double().sum(-1) - 1).abs().max()) <= 4e-7 * 4
    assert float(all_attn_per_head.max() - all_attn_per_head.min()) > 0.05
    assert len(capture.qk) == 2 and len(band_embeds) == 8
    assert all(torch.equal(a, b) for a, b in zip(plain, observed))
    assert set(plain[0].unique().tolist()) <= {-1.0, 1.0}
