"""The attention maps of the band-attention head on the GPU: wv_band_attn_maps (csrc/head_attn.hip) against the
reference-made fixture tests/golden/head_attn_golden.npz, the fp64 truth and the host twin (tests/head_attn_cases.py: truth,
tolerance), over the shapes at which the kernel or its GEMMs take another path, with guard values behind every output, and
GPU heads whose `attn` submodule is observed.

Measured on MI355X, error over e_ref (the fixture's own error against the fp64 truth) over the 13 cases and both layouts:
probs 0.68 - 1.71 x, scores 0.81 - 1.39 x e_scores32, attn_out 0.42 - 1.24 x on nine cases and 3.3 - 4.2 x on the four E = 384, B = 3
cases, whose e_ref is 3.9e-7: errors of 1.3e-6 - 1.7e-6, inside the 4e-6 floor.  Kernel - twin: at most 1.5e-5 (probs), 2.3e-5
(attn_out), 7.2e-5 (scores), all at factor 100.  The bound is 4 x e_ref or the floor."""
import ctypes

import pytest
import torch

import head_attn_cases as hac
from wvhash import _lib
from wvhash.models import fusion

pytestmark = pytest.mark.gpu

GUARD = 64          # floats behind every output buffer
OUTPUTS = ("probs", "probs_mean", "scores", "attn_out")


def raw_maps(head, kv, layout, S, B, want=OUTPUTS, q_proj=False):
    """wv_band_attn_maps through the C ABI on a GPU head and GPU tokens: dict of host tensors.  Every output buffer is
    followed by GUARD floats of 7.0, which must still be there afterwards.  q_proj: hand in queries projected ahead of time
    by wv_band_attn_qproj."""
    lib = _lib.require_gpu()
    E, H = head.attn.embed_dim, head.attn.num_heads
    q_eff = head.effective_queries().detach().float().reshape(-1, E).contiguous()
    Nq = q_eff.shape[0]
    p, keep = fusion._head_params(S, E, q_eff, head.attn, head.norm1, head.norm2, head.mlp[0], head.mlp[2], head.out_proj, False)
    if q_proj:
        qp = torch.empty_like(q_eff)
        _lib.check(lib.wv_band_attn_qproj(ctypes.byref(p), _lib.ptr(qp), _lib.stream_ptr()), "wv_band_attn_qproj")
        p.q_proj = qp.data_ptr()
    shapes = dict(probs=(B, H, Nq, S), probs_mean=(B, Nq, S), scores=(B, H, Nq, S), attn_out=(B, Nq, E))
    bufs = {}
    for name in want:
        n = 1
        for d in shapes[name]:
            n *= d
        bufs[name] = torch.full((n + GUARD,), 7.0, device="cuda")
    need = lib.wv_band_attn_maps_workspace_bytes(ctypes.byref(p), B)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.wv_band_attn_maps(ctypes.byref(p), _lib.ptr(kv), fusion._LAYOUTS[layout], B, *[_lib.ptr(bufs.get(n)) for n in OUTPUTS],
                               _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream_ptr())
    _lib.check(rc, "wv_band_attn_maps")
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu()
        assert bool((host[-GUARD:] == 7.0).all()), f"{name}: written past its extent"
        out[name] = host[:-GUARD].reshape(shapes[name])
    return out


@pytest.mark.parametrize("layout", ["bse", "sbe"])
@pytest.mark.parametrize("name", hac.NAMES)
def test_kernel_against_fixture_truth_and_twin(name, layout):
    c = hac.case(name)
    head = c.module()
    kv = c.kv if layout == "bse" else c.kv.transpose(0, 1).contiguous()
    twin = fusion.band_attn_maps(kv, head.effective_queries(), head.attn, layout)
    head = head.cuda()
    got = fusion.band_attn_maps(kv.cuda(), head.effective_queries(), head.attn, layout)
    assert all(t.is_cuda for t in got)
    got = fusion.AttnMaps(*[t.cpu() for t in got])
    c.check(got, f"kernel/{layout}")
    assert float((got.weights.double().sum(-1) - 1).abs().max()) <= 4e-7 * 4
    for label, a, b, tol in (("probs", got.weights, twin.weights, c.tol_probs), ("attn_out", got.attn_output, twin.attn_output, c.tol_out),
                             ("scores", got.scores, twin.scores, c.tol_scores)):
        d = float((a.double() - b.double()).abs().max())
        print(f"kernel - twin {name} {label}: {d:.3e} (tol {tol:.3e})")
        assert d <= tol, (name, label, d, tol)
    mean = fusion.band_attn_maps(kv.cuda(), head.effective_queries(), head.attn, layout, per_head=False, want=("probs",))
    c.check(fusion.AttnMaps(mean.weights.cpu(), None, None), f"kernel/{layout}/mean", per_head=False)


SHAPES = {                                  # E, heads, Nq, S, B
    "B1": (384, 8, 4, 4, 1),                # S B = 4 rows: the small-M GEMM
    "B3": (384, 8, 4, 4, 3),
    "B257": (384, 8, 4, 4, 257),            # S B = 1028: ragged tiles
    "S1": (64, 8, 4, 1, 5),                 # every probability is exactly 1.0
    "S5": (64, 8, 4, 5, 5),
    "S64_E64": (64, 8, 4, 64, 3),
    "S24_E384": (384, 8, 4, 24, 2),         # 77 KB of LDS: beyond the 64 KB a kernel gets without asking
    "Nq1": (384, 8, 1, 4, 3),
    "Nq8": (384, 8, 8, 4, 3),
    "Nq64": (64, 8, 64, 4, 3),              # Nq H S = 2048 dot products: more than the workgroup
    "H1_E96": (96, 1, 4, 4, 3),             # head dimension 96
    "H8_E64": (64, 8, 4, 4, 3),             # head dimension 8
}


@pytest.mark.parametrize("layout", ["bse", "sbe"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_against_the_fp64_truth(shape, layout):
    """Each shape against stock nn.MultiheadAttention in fp64; e_ref is the fp32 stock module's own error at the shape (the
    fixture has none for it).  Guard values behind every output; with and without queries projected ahead of time."""
    E, heads, nq, S, B = SHAPES[shape]
    sc = hac.shape_case(E, heads, nq, S, B)
    head = hac.shape_module(E, heads, nq, sc["sd"]).cuda()
    kv = (sc["kv"] if layout == "bse" else sc["kv"].transpose(0, 1).contiguous()).cuda()
    out = raw_maps(head, kv, layout, S, B)
    for label, got, truth in (("probs", out["probs"], sc["probs"]), ("probs", out["probs_mean"], sc["probs"].mean(1)),
                              ("scores", out["scores"], sc["scores"]), ("attn_out", out["attn_out"], sc["attn_out"])):
        err = float((got.double() - truth).abs().max())
        print(f"{shape}/{layout} {label}{tuple(got.shape)}: err {err:.3e}, tol {sc['tol'][label]:.3e}")
        assert err <= sc["tol"][label], (shape, label, err)
    assert float((torch.softmax(out["scores"], -1) - out["probs"]).abs().max()) <= sc["tol"]["probs"]
    assert float((out["probs"].double().sum(-1) - 1).abs().max()) <= 4e-7 * S
    if S == 1:
        assert bool((out["probs"] == 1.0).all()) and bool((out["probs_mean"] == 1.0).all())
    ahead = raw_maps(head, kv, layout, S, B, q_proj=True)
    assert all(torch.equal(out[n], ahead[n]) for n in OUTPUTS)


def test_subsets_of_outputs_and_their_guards():
    """Any subset of the outputs: calls that project V (attn_out asked for) agree bit for bit among themselves, as do the calls
    that project K alone; between the two groups the K columns come from products of different widths, so those are held
    to the tolerance."""
    c = hac.case("adv_e384_nq4_x4")
    head = c.module().cuda()
    kv = c.kv.cuda()
    full = raw_maps(head, kv, "bse", 4, c.B)
    k_only = raw_maps(head, kv, "bse", 4, c.B, want=("probs", "probs_mean", "scores"))
    for want in (("attn_out",), ("probs", "attn_out"), ("scores", "attn_out"), ("probs_mean", "attn_out")):
        got = raw_maps(head, kv, "bse", 4, c.B, want=want)
        assert all(torch.equal(got[n], full[n]) for n in want), want
    for want in (("probs",), ("probs_mean",), ("scores",), ("probs", "scores")):
        got = raw_maps(head, kv, "bse", 4, c.B, want=want)
        assert all(torch.equal(got[n], k_only[n]) for n in want), want
    c.check(fusion.AttnMaps(k_only["probs"], k_only["scores"], None), "kernel/K only")
    assert float((k_only["probs"] - full["probs"]).abs().max()) <= c.tol_probs


def test_tokens_that_do_not_fit_the_lds_are_refused():
    """S = 64 at E = 384: wv_band_attn_pool's refusal, and the module answers such a call with stock PyTorch."""
    E, heads, nq, S, B = 384, 8, 4, 64, 2
    sc = hac.shape_case(E, heads, nq, S, B)
    head = hac.shape_module(E, heads, nq, sc["sd"]).cuda()
    with pytest.raises(_lib.WvhashUnsupported, match="64 tokens x 4 queries at embed_dim=384 do not fit"):
        fusion.band_attn_maps(sc["kv"].cuda(), head.effective_queries(), head.attn)
    q = head.effective_queries().detach().expand(B, -1, -1)
    with torch.no_grad():
        out, w = head.attn(q, sc["kv"].cuda(), sc["kv"].cuda(), average_attn_weights=False)
    assert float((w.cpu().double() - sc["probs"]).abs().max()) < 1e-5


@pytest.mark.parametrize("front", [None, "0", "1"])
@pytest.mark.parametrize("name", ["adv_e384_nq4_x4", "decoupled_e384_nq4", "adv_e64_nq4"])
def test_observed_gpu_head(name, front, diag, monkeypatch):
    """The hook, keyword pre-hook and patched forward of the collapse study on a GPU head in eval mode, by dispatch and with
    either front pinned on the diagnostic library: per-head weights and the (query, key) of the call arrive, the head's output
    keeps its bits, and the unobserved forward calls neither `attn` nor wv_band_attn_maps."""
    if front is None:
        diag.delenv("WV_HEAD_FRONT", raising=False)
    else:
        diag.setenv("WV_HEAD_FRONT", front)
    c = hac.case(name)
    head = c.module().cuda()
    feats = [f.cuda() for f in c.feats]
    counter = hac.CallCounter(monkeypatch)
    with torch.no_grad():
        plain = head(feats)
    assert counter.attn_calls == 0 and counter.lib_calls == 0
    observed, cap = hac.observe(head, lambda: head(feats))
    assert torch.equal(plain, observed) and counter.attn_calls == 1 and counter.lib_calls == 1
    (w,), (out,), ((q, k),) = cap.weights, cap.outputs, cap.qk
    assert tuple(w.shape) == (c.B, 8, c.nq, 4) and tuple(q.shape) == (c.B, c.nq, c.E) and torch.equal(k, c.kv)
    c.check(fusion.AttnMaps(w, None, out), f"observed GPU head front={front}")
    with torch.no_grad():
        again = head(feats)
    assert torch.equal(plain, again) and counter.attn_calls == 1 and counter.lib_calls == 1
    if name == "adv_e384_nq4_x4" and front is None:
        got = []
        handle = head.attn.register_forward_hook(lambda module, inputs, output: got.append(output[1]))
        head.matrix_dtype = "bf16"                     # the maps stay the fp32 attention of the same tokens
        with torch.no_grad():
            head(feats)
        handle.remove()
        assert tuple(got[0].shape) == (c.B, c.nq, 4) and got[0].is_cuda
        assert float((got[0] - head.attention_maps(feats)).abs().max()) <= c.tol_probs
        c.check(fusion.AttnMaps(got[0].cpu(), None, None), "plain hook, bf16 head", per_head=False)


def test_train_mode_stays_stock_pytorch(monkeypatch):
    c = hac.case("adv_e64_nq4")
    head = c.module().cuda().train()
    counter = hac.CallCounter(monkeypatch)
    got = []
    handle = head.attn.register_forward_hook(lambda module, inputs, output: got.append(output[1]))
    y = head([f.cuda() for f in c.feats])
    handle.remove()
    assert counter.attn_calls == 1 and counter.lib_calls == 0
    assert y.requires_grad and got[0].requires_grad and tuple(got[0].shape) == (c.B, c.nq, 4)
