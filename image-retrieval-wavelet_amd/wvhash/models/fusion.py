"""Band-attention fusion heads: module names, constructor kwargs and state_dict keys of
/root/reference/main/models/multi_dino_attention.py (CrossAttentionBottleneckHead :1001-1062,
...Advanced :1064-1141, ...Pooled :484-599, ...Decoupled :336-481, get_fusion_head :602-690).

Eval-mode forward on GPU tensors runs the HIP/MFMA kernels (wv_band_attn_pool; with `head.matrix_dtype = "bf16"` or
"auto" the opt-in bf16 matrix-core path, wv_band_attn_pool_bf16).  Training-mode
forward (dropout, autograd, ortho loss) is stock PyTorch on the GPU: training is outside the
accelerated path.  There is no CPU execution path.

The fused forward never calls `head.attn`.  A head whose `attn` carries a forward hook, a forward pre-hook or a patched
`forward` (the reference's attention.py and studies/measure_attention_collapse.py read the head that way) makes that call
as well, once per forward, and the module answers it from wv_band_attn_maps (BandMultiheadAttention); the head's own
result still comes from wv_band_attn_pool, so an observer never changes a code bit.
"""
import collections
import ctypes
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ._prepared import PreparedCache, param_key

LOGGER = logging.getLogger("RETRIEVAL")


def _stacked(features_list, keep_bf16=False):
    """S x [B, E] -> one [S, B, E] fp32 tensor.  Band features that already lie back to back in one allocation
    (slices of a preallocated [S, B, E] buffer the backbones wrote into) are used in place, without a copy.
    keep_bf16 (the bf16 head): features that are all bf16 stay bf16 -- in place or stacked, never upcast."""
    f0 = features_list[0]
    dtype = torch.bfloat16 if keep_bf16 and all(f.dtype == torch.bfloat16 for f in features_list) else torch.float32
    if f0.dtype == dtype and f0.dim() == 2 and f0.is_contiguous():
        base, step = f0.untyped_storage().data_ptr(), f0.numel() * f0.element_size()
        if all(f.dtype == dtype and f.shape == f0.shape and f.is_contiguous()
               and f.untyped_storage().data_ptr() == base and f.data_ptr() == f0.data_ptr() + i * step
               for i, f in enumerate(features_list)):
            return f0.as_strided((len(features_list),) + tuple(f0.shape), (f0.numel(), f0.shape[1], 1))
    return torch.stack([f.to(dtype) for f in features_list], dim=0).contiguous()


def resolve_matrix_dtype(value, device_type="cuda"):
    """`matrix_dtype` of a head or a call -> None (the fp32 matrix-core path) or "bf16".  Accepted: None, torch.bfloat16 /
    "bf16" / "bfloat16", and "auto" = bf16 exactly when the call runs under torch.autocast(device_type, dtype=torch.bfloat16)."""
    if value is None:
        return None
    if value is torch.bfloat16 or value in ("bf16", "bfloat16"):
        return "bf16"
    if isinstance(value, str) and value == "auto":
        return "bf16" if torch.is_autocast_enabled(device_type) and torch.get_autocast_dtype(device_type) == torch.bfloat16 else None
    raise ValueError(f"matrix_dtype must be None, torch.bfloat16 / 'bf16' or 'auto', got {value!r}")


def _head_params(S, E, q_eff, attn, norm1, norm2, mlp0, mlp2, out_proj, pool_mean):
    """_lib.HeadParams of the module's parameters (no projected queries, no prepared blob), and the fp32 contiguous
    tensors its pointers refer to: the caller keeps them alive for the call."""
    keep = [t.detach().float().contiguous() for t in
            (q_eff, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight, attn.out_proj.bias, norm1.weight, norm1.bias,
             mlp0.weight, mlp0.bias, mlp2.weight, mlp2.bias, out_proj.weight, out_proj.bias, norm2.weight, norm2.bias)]
    p = _lib.HeadParams()
    p.embed_dim, p.num_heads, p.num_queries, p.num_tokens = E, attn.num_heads, q_eff.shape[0], S
    p.pool_mean = 1 if pool_mean else 0
    (p.q_eff, p.in_proj_w, p.in_proj_b, p.attn_out_w, p.attn_out_b, p.norm1_w, p.norm1_b, p.mlp0_w, p.mlp0_b,
     p.mlp2_w, p.mlp2_b, p.out_w, p.out_b, p.norm2_w, p.norm2_b) = [t.data_ptr() for t in keep]
    p.ln_eps = float(norm1.eps)
    p.q_proj = None
    p.prepared = None
    return p, keep


Prepared = collections.namedtuple("Prepared", "blob qp")


def _prepared_key(query_key, q_src, watched, *config):
    """Key of what is prepared from the parameters: the identity of what q_eff was made from (query_key; by default q_eff
    itself), of the watched weights, and the configuration the layout depends on."""
    return (query_key if query_key is not None else param_key(q_src), param_key(*watched)) + config


def band_attn_pool(features_list, q_eff, attn, norm1, norm2, mlp0, mlp2, out_proj, pool_mean=False,
                   cache=None, query_key=None, matrix_dtype=None, workspace=None):
    """HIP forward of the attention-pooling core.  features_list: S x [B, E] CUDA fp32.
    matrix_dtype: None = the fp32 matrix-core path; torch.bfloat16 / "bf16" / "auto" (see resolve_matrix_dtype) = the bf16
    path (wv_band_attn_pool_bf16: bf16 operands, fp32 accumulation, fp32 output), which also takes bf16 features as they
    are.
    cache: the module's PreparedCache; holds, per device, what is made from parameters alone, so that it is rebuilt when a
    parameter changes, not in every call.  Slot "fp32": the projected query tokens (`qp`) or, for the configurations with a
    one-launch front (wv_band_attn_prepared_bytes), the fragment-ordered copy of the weights (`blob`); slot "bf16": that
    path's prepared blob -- separate slots, so that alternating precisions rebuilds neither.  Without a cache nothing is
    kept: the fp32 path projects the queries in the call, the bf16 path builds a blob for this call alone.
    query_key identifies the parameters q_eff was made from (param_key).
    workspace: a caller-owned uint8 buffer for this one call; by default a fresh allocation of the advertised size."""
    lib = _lib.require_gpu()
    use_bf16 = resolve_matrix_dtype(matrix_dtype) == "bf16"
    feats = _stacked(features_list, keep_bf16=use_bf16)                               # [S, B, E]
    S, B, E = feats.shape
    dev = feats.device
    q_src = q_eff
    q_eff = q_eff.detach().float().reshape(-1, E).contiguous()
    p, keep = _head_params(S, E, q_eff, attn, norm1, norm2, mlp0, mlp2, out_proj, pool_mean)
    for t in keep:
        if not t.is_cuda:
            raise ValueError("band_attn_pool: module parameters must live on the GPU")
    out = torch.empty((B, E), dtype=torch.float32, device=dev)
    if B == 0:
        return out
    # the query tokens and the weights are parameters: key on their storage and version counters
    watched = (attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight, mlp0.weight, mlp2.weight)
    if use_bf16:
        key = _prepared_key(query_key, q_src, watched + (out_proj.weight,), attn.num_heads, S, p.pool_mean)
        return _band_attn_pool_bf16(lib, p, feats, out, workspace, cache, key)
    if cache is not None:
        def build():
            with torch.cuda.device(dev):
                nbytes = lib.wv_band_attn_prepared_bytes(ctypes.byref(p))
                if nbytes:      # this configuration has the one-launch front: projected queries + fragment-ordered weights
                    blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    _lib.check(lib.wv_band_attn_prepare(ctypes.byref(p), _lib.ptr(blob), _lib.stream_ptr()), "wv_band_attn_prepare")
                    return Prepared(blob, None)
                qp = torch.empty_like(q_eff)
                _lib.check(lib.wv_band_attn_qproj(ctypes.byref(p), _lib.ptr(qp), _lib.stream_ptr()), "wv_band_attn_qproj")
                return Prepared(None, qp)
        prepared = cache.get("fp32", dev, _prepared_key(query_key, q_src, watched, attn.num_heads, S), build)
        if prepared.blob is not None:
            p.prepared = prepared.blob.data_ptr()
        else:
            p.q_proj = prepared.qp.data_ptr()
    ws_bytes = lib.wv_band_attn_pool_workspace_bytes(ctypes.byref(p), B)
    if workspace is None or workspace.numel() < ws_bytes or workspace.device != dev:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.wv_band_attn_pool(ctypes.byref(p), _lib.ptr(feats), B, _lib.ptr(out), _lib.ptr(workspace),
                                   ctypes.c_size_t(workspace.numel()), _lib.stream_ptr())
        _lib.check(rc, "wv_band_attn_pool")
    return out


def _band_attn_pool_bf16(lib, p, feats, out, workspace, cache, key):
    """The bf16 matrix-core path: prepared blob (projected queries + bf16 weights) from `cache`, then one call."""
    S, B, E = feats.shape
    dev = feats.device

    def build():
        with torch.cuda.device(dev):
            nbytes = lib.wv_band_attn_bf16_prepared_bytes(ctypes.byref(p))
            if not nbytes:      # never a silent fp32 run
                raise _lib.WvhashError("wv_band_attn_bf16_prepared_bytes: " + lib.wv_last_error().decode(errors="replace"))
            blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.wv_band_attn_bf16_prepare(ctypes.byref(p), _lib.ptr(blob), _lib.stream_ptr()), "wv_band_attn_bf16_prepare")
        return Prepared(blob, None)
    blob = (cache.get("bf16", dev, key, build) if cache is not None else build()).blob
    ws_bytes = lib.wv_band_attn_pool_bf16_workspace_bytes(ctypes.byref(p), B)
    if workspace is None or workspace.numel() < ws_bytes or workspace.device != dev:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dt = _lib.WV_DT_BF16 if feats.dtype == torch.bfloat16 else _lib.WV_DT_F32
    with torch.cuda.device(dev):
        rc = lib.wv_band_attn_pool_bf16(ctypes.byref(p), _lib.ptr(blob), _lib.ptr(feats), dt, B, _lib.ptr(out), _lib.ptr(workspace),
                                        ctypes.c_size_t(workspace.numel()), _lib.stream_ptr())
        _lib.check(rc, "wv_band_attn_pool_bf16")
    return out


def band_attn_pool_host(features_list, q_eff, attn, norm1, norm2, mlp0, mlp2, out_proj, pool_mean=False, matrix_dtype=None):
    """The same forward on HOST tensors through the library's host twin (wv_band_attn_pool_cpu, csrc/host_head.cpp): for a
    model that was moved to the CPU on purpose.  fp32, machine-independent summation order; agrees with the kernels to
    fp32 rounding.  matrix_dtype as in band_attn_pool: "bf16" runs wv_band_attn_pool_bf16_cpu (operands of the weight
    products rounded to bf16, everything else as here; bf16 features are read as they are)."""
    lib = _lib.load()
    use_bf16 = resolve_matrix_dtype(matrix_dtype, "cpu") == "bf16"
    fdt = torch.bfloat16 if use_bf16 and all(f.dtype == torch.bfloat16 for f in features_list) else torch.float32
    feats = torch.stack([f.detach().to(fdt) for f in features_list], dim=0).contiguous()        # [S, B, E]
    S, B, E = feats.shape
    q_eff = q_eff.detach().float().reshape(-1, E).contiguous()
    p, keep = _head_params(S, E, q_eff, attn, norm1, norm2, mlp0, mlp2, out_proj, pool_mean)
    if any(t.is_cuda for t in keep) or feats.is_cuda:
        raise ValueError("band_attn_pool_host takes host tensors (features and parameters)")
    out = torch.empty((B, E), dtype=torch.float32)
    if use_bf16:
        dt = _lib.WV_DT_BF16 if fdt == torch.bfloat16 else _lib.WV_DT_F32
        _lib.check(lib.wv_band_attn_pool_bf16_cpu(ctypes.byref(p), _lib.ptr(feats), dt, B, _lib.ptr(out)), "wv_band_attn_pool_bf16_cpu")
        return out
    _lib.check(lib.wv_band_attn_pool_cpu(ctypes.byref(p), _lib.ptr(feats), B, _lib.ptr(out)), "wv_band_attn_pool_cpu")
    return out


AttnMaps = collections.namedtuple("AttnMaps", "weights scores attn_output")
_LAYOUTS = {"sbe": _lib.WV_TOKENS_SBE, "bse": _lib.WV_TOKENS_BSE}


def band_attn_maps(kv, q_eff, attn, layout="bse", per_head=True, want=("probs", "scores", "attn_out")):
    """What `attn(query=q_eff broadcast over the batch, key=kv, value=kv)` computes in eval mode, through wv_band_attn_maps
    (GPU tensors) or its host twin (host tensors): AttnMaps(weights, scores, attn_output), None for what `want` leaves out.
    kv: the band tokens, [B, S, E] (layout "bse": torch.stack(kv_list, 1)) or [S, B, E] ("sbe"); q_eff: [Nq, E] or [1, Nq, E].
    weights ("probs"): the softmax, [B, H, Nq, S] with per_head, else its mean over the heads [B, Nq, S]; scores: what the
    softmax is taken of, [B, H, Nq, S]; attn_output ("attn_out"): out_proj(context), [B, Nq, E].  Always fp32 arithmetic:
    bf16 tokens are upcast, and under matrix_dtype="bf16" these are the fp32 attention of the same parameters and tokens,
    not the bf16 path's internal values."""
    if layout not in _LAYOUTS:
        raise ValueError(f"band_attn_maps: layout must be 'bse' or 'sbe', got {layout!r}")
    want = tuple(want)
    if not want or set(want) - {"probs", "scores", "attn_out"}:
        raise ValueError(f"band_attn_maps: want must name some of 'probs', 'scores', 'attn_out', got {want!r}")
    if kv.dim() != 3:
        raise ValueError(f"band_attn_maps: kv must be [B, S, E] or [S, B, E], got {tuple(kv.shape)}")
    kv = kv.detach().float().contiguous()
    E = kv.shape[2]
    B, S = (kv.shape[0], kv.shape[1]) if layout == "bse" else (kv.shape[1], kv.shape[0])
    keep = [t.detach().float().contiguous() for t in
            (q_eff.reshape(-1, E), attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight, attn.out_proj.bias)]
    if any(t.device != kv.device for t in keep):
        raise ValueError("band_attn_maps: the module's parameters and the query tokens must live where kv does")
    p = _lib.HeadParams()                                    # every pointer the maps do not read stays NULL
    p.embed_dim, p.num_heads, p.num_queries, p.num_tokens = E, attn.num_heads, keep[0].shape[0], S
    p.q_eff, p.in_proj_w, p.in_proj_b, p.attn_out_w, p.attn_out_b = [t.data_ptr() for t in keep]
    H, Nq = p.num_heads, p.num_queries

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=kv.device)
    weights = (new(B, H, Nq, S) if per_head else new(B, Nq, S)) if "probs" in want else None
    scores = new(B, H, Nq, S) if "scores" in want else None
    attn_out = new(B, Nq, E) if "attn_out" in want else None
    _lib.wv_band_attn_maps(p, kv, _LAYOUTS[layout], B, probs=weights if per_head else None,
                           probs_mean=None if per_head else weights, scores=scores, attn_out=attn_out)
    return AttnMaps(weights, scores, attn_out)


class BandMultiheadAttention(nn.MultiheadAttention):
    """nn.MultiheadAttention -- same parameters, same state_dict keys -- whose eval-mode forward answers the heads' call
    (batch-broadcast queries attending over a few band tokens, key is value, no masks, fp32) from the library:
    wv_band_attn_maps on the GPU, its host twin on the host.  Every other call (training mode, masks, distinct key and
    value, per-sample queries, other dtypes, tensors that need autograd, shapes outside the kernel) is stock PyTorch."""

    def _library_takes(self, query, key, value, key_padding_mask, attn_mask, is_causal):
        if (self.training or not self.batch_first or not self._qkv_same_embed_dim or self.in_proj_bias is None
                or self.bias_k is not None or self.add_zero_attn):
            return False
        if key_padding_mask is not None or attn_mask is not None or is_causal or key is not value:
            return False
        if query.dim() != 3 or key.dim() != 3 or query.shape[0] != key.shape[0] or query.shape[0] == 0:
            return False
        if not (query.stride(0) == 0 or query.shape[0] == 1):                 # one set of queries for the whole batch
            return False
        E = self.embed_dim
        if query.shape[2] != E or key.shape[2] != E or E % 8 or not (1 <= query.shape[1] <= 64 and 1 <= key.shape[1] <= 64):
            return False
        if query.dtype != torch.float32 or key.dtype != torch.float32:
            return False
        if not (query.device == key.device == self.in_proj_weight.device) or key.device.type not in ("cuda", "cpu"):
            return False
        return not (torch.is_grad_enabled() and (query.requires_grad or key.requires_grad))

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None,
                average_attn_weights=True, is_causal=False):
        if self._library_takes(query, key, value, key_padding_mask, attn_mask, is_causal):
            try:
                maps = band_attn_maps(key, query[0], self, "bse", per_head=not average_attn_weights,
                                      want=("probs", "attn_out") if need_weights else ("attn_out",))
                return maps.attn_output, maps.weights
            except _lib.WvhashUnsupported:                                     # WV_ENOTSUP: more tokens than fit the kernel's LDS
                pass
        return super().forward(query, key, value, key_padding_mask=key_padding_mask, need_weights=need_weights,
                               attn_mask=attn_mask, average_attn_weights=average_attn_weights, is_causal=is_causal)


class CrossAttentionBottleneckHeadAdvanced(nn.Module):
    _pool = "concat"

    def __init__(self, input_dims, embed_dim=384, num_queries=4, num_heads=8, dropout=0.1,
                 sub_band_dropout_p=0.3, ortho_weight=0.1, margin=0.0, use_all_tokens=False):
        super().__init__()
        self.num_queries = num_queries
        self.sub_band_dropout_p = sub_band_dropout_p
        self.ortho_weight = ortho_weight
        self.margin = margin
        self.use_all_tokens = use_all_tokens
        self.projections = nn.ModuleList([
            nn.Linear(dim, embed_dim) if dim != embed_dim else nn.Identity() for dim in input_dims
        ])
        self.query_tokens = nn.Parameter(torch.randn(1, num_queries, embed_dim))
        nn.init.trunc_normal_(self.query_tokens, std=0.02)
        self.attn = BandMultiheadAttention(embed_dim, num_heads, dropout=dropout, batch_first=True)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.mlp = nn.Sequential(
            nn.Linear(embed_dim, embed_dim * 4), nn.GELU(),
            nn.Linear(embed_dim * 4, embed_dim), nn.Dropout(dropout)
        )
        in_dim = embed_dim if self._pool == "mean" else num_queries * embed_dim
        self.out_proj = nn.Linear(in_dim, embed_dim)
        self.last_ortho_loss = 0.0
        self._zero_loss = None
        self._prepared = PreparedCache()        # slots "fp32" and "bf16" (band_attn_pool); shared with replicas, on purpose
        # None: fp32 matrix cores (default); torch.bfloat16 / "bf16": the bf16 path; "auto": bf16 under bf16 autocast
        self.matrix_dtype = None

    # -- pieces shared by the four variants ------------------------------------------------
    def compute_ortho_loss(self):
        Q = self.query_tokens.squeeze(0)
        Q_norm = F.normalize(Q, p=2, dim=-1)
        gram = torch.matmul(Q_norm, Q_norm.T)
        identity = torch.eye(self.num_queries, device=Q.device)
        raw_error = torch.norm(gram - identity, p='fro')
        active_error = F.relu(raw_error - self.margin)
        return self.ortho_weight * (active_error ** 2)

    def effective_queries(self):
        return self.query_tokens

    def _query_key(self):
        """Identity of the parameters effective_queries() is made from (for the cached query projection)."""
        return param_key(self.query_tokens)

    def _ortho_after_attention(self, attn_weights, mask_ll, device):
        if self.training and self.ortho_weight > 0:
            return self.compute_ortho_loss()
        return torch.zeros((), device=device)

    def _readout(self, x, batch_size):
        return x.mean(dim=1) if self._pool == "mean" else x.view(batch_size, -1)

    def _hip_ok(self, kv_list):
        """Eval mode, CLS tokens only ([B, E] per band), nothing that needs autograd."""
        if self.training or self.use_all_tokens or len(kv_list) > 64:
            return False
        if any(t.dim() != 2 or not t.is_cuda for t in kv_list):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in kv_list))

    def _attn_observed(self):
        """Someone reads this head through its `attn` submodule: a forward hook, a forward pre-hook or an instance-level
        `forward` (module-global hooks, nn.modules.module.register_module_forward_hook, are not looked at)."""
        a = self.attn
        if a._forward_hooks or a._forward_pre_hooks:
            return True
        # a patch that was "restored" with setattr leaves the class's own bound method in the instance: no override
        f = vars(a).get("forward")
        return f is not None and not (getattr(f, "__self__", None) is a and getattr(f, "__func__", None) is type(a).forward)

    def _observe_attention(self, kv_list, batch_size):
        """The call the reference's forward makes on `attn`, through nn.Module.__call__ so that its observers fire; the
        module computes it with wv_band_attn_maps / the host twin (BandMultiheadAttention).  The result is theirs alone."""
        if batch_size == 0:
            return
        with torch.no_grad():
            q = self.effective_queries().float().expand(batch_size, -1, -1)
            kv = torch.stack([t.float() for t in kv_list], dim=1)
            self.attn(query=q, key=kv, value=kv)

    def attention_maps(self, features_list, per_head=False, scores=False):
        """The attention of this head over the bands of `features_list` (S x [B, dim]), without hooks: the softmax weights
        [B, Nq, S] (per_head: [B, H, Nq, S]); with scores=True the pair (weights, pre-softmax scores [B, H, Nq, S]).  Eval-mode
        values (no dropout, no LL masking) in fp32 whatever `matrix_dtype` is; GPU tensors or, through the host twin, host
        tensors."""
        with torch.no_grad():
            kv_list = [proj(f) for proj, f in zip(self.projections, features_list)]
            if any(t.dim() != 2 for t in kv_list):
                raise ValueError("attention_maps covers CLS-token inputs ([B, dim] per band)")
            maps = band_attn_maps(torch.stack([t.float() for t in kv_list], dim=0), self.effective_queries(), self.attn, "sbe",
                                  per_head=per_head, want=("probs", "scores") if scores else ("probs",))
        return (maps.weights, maps.scores) if scores else maps.weights

    def forward(self, features_list):
        batch_size = features_list[0].shape[0]
        device = features_list[0].device
        kv_list = [proj(f) for proj, f in zip(self.projections, features_list)]
        if not features_list[0].is_cuda and not self.training:
            # host tensors: never a silent fallback -- only after an explicit `head.host_twin = True` (a model meant to run
            # on the CPU) does the library's host twin take the eval-mode forward (same math, fp32)
            if not getattr(self, "host_twin", False):
                raise _lib.WvhashUnavailable("the eval-mode fusion head runs on the GPU; for a model that is meant to run on "
                                             "the host set `head.host_twin = True` (wv_band_attn_pool_cpu) -- there is no "
                                             "silent CPU fallback.  The training-mode forward is stock PyTorch and follows "
                                             "its tensors' device")
            if (self.use_all_tokens or len(kv_list) > 64 or any(t.dim() != 2 for t in kv_list)
                    or self.norm1.normalized_shape[0] % 8 or next(self.parameters()).is_cuda):
                raise _lib.WvhashUnavailable("the eval-mode fusion head on host tensors covers CLS-token inputs ([B, E] per "
                                             "band, E a multiple of 8, at most 64 bands) of a model that lives on the host")
            self.last_ortho_loss = torch.zeros(())
            if self._attn_observed():
                self._observe_attention(kv_list, batch_size)
            with torch.no_grad():
                return band_attn_pool_host(kv_list, self.effective_queries(), self.attn, self.norm1, self.norm2,
                                           self.mlp[0], self.mlp[2], self.out_proj, self._pool == "mean",
                                           matrix_dtype=self.matrix_dtype)

        if self._hip_ok(kv_list):
            # torch.zeros launches a fill on the stream; torch.tensor(0.0, device=...) is a blocking host-to-device
            # copy that drains everything queued before it (here: the whole SWT kernel of the step)
            if self._zero_loss is None or self._zero_loss.device != device:
                self._zero_loss = torch.zeros((), device=device)
            self.last_ortho_loss = self._zero_loss
            if self._attn_observed():
                self._observe_attention(kv_list, batch_size)
            with torch.no_grad():
                out = band_attn_pool(kv_list, self.effective_queries(), self.attn, self.norm1, self.norm2,
                                     self.mlp[0], self.mlp[2], self.out_proj, self._pool == "mean", self._prepared,
                                     self._query_key(), matrix_dtype=self.matrix_dtype)
            return out

        # training / unsupported shapes: stock PyTorch on the GPU (outside the accelerated path)
        mask_ll = self.training and (torch.rand(1).item() < self.sub_band_dropout_p)
        if mask_ll:
            kv_list[0] = torch.zeros_like(kv_list[0])
        kv = torch.cat(kv_list, dim=1) if self.use_all_tokens else torch.stack(kv_list, dim=1)
        q = self.effective_queries().expand(batch_size, -1, -1)
        attn_output, attn_weights = self.attn(query=q, key=kv, value=kv)
        self.last_ortho_loss = self._ortho_after_attention(attn_weights, mask_ll, device)
        x = self.norm1(q + attn_output)
        x = x + self.mlp(x)
        x = self._readout(x, batch_size)
        x = self.out_proj(x)
        return self.norm2(x)


class CrossAttentionBottleneckHead(CrossAttentionBottleneckHeadAdvanced):
    """Ortho loss on the attention weights instead of the query Gram (:1047-1052)."""

    def __init__(self, input_dims, embed_dim=384, num_queries=4, num_heads=8, dropout=0.1,
                 sub_band_dropout_p=0.3, ortho_weight=0.1, use_all_tokens=False):
        super().__init__(input_dims, embed_dim, num_queries, num_heads, dropout, sub_band_dropout_p,
                         ortho_weight, 0.0, use_all_tokens)

    def _ortho_after_attention(self, attn_weights, mask_ll, device):
        if mask_ll or not self.training:
            return torch.tensor(0.0, device=device, requires_grad=True)
        M = attn_weights.mean(dim=0)
        identity = torch.eye(self.num_queries, device=device)
        return self.ortho_weight * (torch.norm(M @ M.t() - identity, p='fro') ** 2)


class CrossAttentionBottleneckHeadPooled(CrossAttentionBottleneckHeadAdvanced):
    def __init__(self, input_dims, embed_dim=384, num_queries=4, num_heads=8, dropout=0.1,
                 sub_band_dropout_p=0.3, ortho_weight=0.1, margin=0.0, use_all_tokens=False,
                 query_pool='mean'):
        if query_pool not in ('mean', 'concat'):
            raise ValueError(f"query_pool must be 'mean' or 'concat', got {query_pool!r}")
        self._pool = query_pool
        self.query_pool = query_pool
        super().__init__(input_dims, embed_dim, num_queries, num_heads, dropout, sub_band_dropout_p,
                         ortho_weight, margin, use_all_tokens)
        self.query_pool = query_pool


class CrossAttentionBottleneckHeadDecoupled(CrossAttentionBottleneckHeadAdvanced):
    def __init__(self, input_dims, embed_dim=384, num_queries=4, num_heads=8, dropout=0.1,
                 sub_band_dropout_p=0.3, ortho_weight=0.1, margin=0.0, use_all_tokens=False,
                 query_scale_init=4.0, normalize_queries=True, learn_query_scale=True):
        super().__init__(input_dims, embed_dim, num_queries, num_heads, dropout, sub_band_dropout_p,
                         ortho_weight, margin, use_all_tokens)
        self.normalize_queries = normalize_queries
        scale = torch.tensor(float(query_scale_init))
        if learn_query_scale:
            self.query_scale = nn.Parameter(scale)
        else:
            self.register_buffer('query_scale', scale)

    def effective_queries(self):
        q = self.query_tokens
        if self.normalize_queries:
            q = F.normalize(q, p=2, dim=-1)
        return q * self.query_scale

    def _query_key(self):
        return param_key(self.query_tokens, self.query_scale) + (self.normalize_queries,)


_HIP_TYPES = {
    'cross_attention_bottleneck': CrossAttentionBottleneckHead,
    'cross_attention_advanced': CrossAttentionBottleneckHeadAdvanced,
    'cross_attention_pooled': CrossAttentionBottleneckHeadPooled,
    'cross_attention_decoupled': CrossAttentionBottleneckHeadDecoupled,
}


def get_fusion_head(fusion_config, output_dims):
    """Same dispatch keys and defaults as the reference (:602-690)."""
    fusion_type = fusion_config.get('type', 'standard')
    embed_dim = fusion_config['output_dim']
    common = dict(
        num_queries=fusion_config.get('num_queries', 4),
        num_heads=fusion_config.get('num_heads', 8),
        dropout=fusion_config.get('dropout', 0.1),
        sub_band_dropout_p=fusion_config.get('sub_band_dropout_p', 0.3),
        ortho_weight=fusion_config.get('ortho_weight', 0.1),
    )
    head = None
    if fusion_type in ('cross_attention_bottleneck', 'cross_attention_advanced'):
        head = _HIP_TYPES[fusion_type](output_dims, embed_dim, **common)
    elif fusion_type == 'cross_attention_pooled':
        head = CrossAttentionBottleneckHeadPooled(
            output_dims, embed_dim, use_all_tokens=fusion_config.get('use_all_tokens', False),
            query_pool=fusion_config.get('query_pool', 'mean'), **common)
    elif fusion_type == 'cross_attention_decoupled':
        head = CrossAttentionBottleneckHeadDecoupled(
            output_dims, embed_dim, use_all_tokens=fusion_config.get('use_all_tokens', False),
            query_scale_init=fusion_config.get('query_scale_init', 4.0),
            normalize_queries=fusion_config.get('normalize_queries', True),
            learn_query_scale=fusion_config.get('learn_query_scale', True), **common)
    if head is not None:
        # optional, absent in every reference YAML: the matrix-core dtype of the eval-mode forward
        head.matrix_dtype = fusion_config.get('matrix_dtype')
        if head.matrix_dtype != "auto":
            resolve_matrix_dtype(head.matrix_dtype)          # an unknown value raises here, not at the first forward
        return head
    # every other type (standard, temperature, semantic, gated, temperature_gated, self_attention, cbam, eca; unknown
    # names fall back to standard like the reference): stock PyTorch modules with the reference's state_dict keys
    from .fusion_extra import build_extra_head
    LOGGER.info("fusion type '%s' runs as stock PyTorch (the HIP head covers the cross-attention family)", fusion_type)
    return build_extra_head(fusion_type, fusion_config, output_dims)
