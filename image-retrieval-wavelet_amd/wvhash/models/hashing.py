"""Wavelet-band hashing models: class names, kwargs and state_dict keys of
/root/reference/main/models/multi_dino_attention.py (SharedDinoHashing :792-833,
MultiDinoHashing :716-750, PromptedSharedDinoHashing :835-899).

Only the tail of these models is on the accelerated path: band split -> [ViT] ->
fusion head (HIP/MFMA) -> hash_fc -> BatchNorm1d -> sign -> bit-pack (HIP).  The DINOv2 backbone
is a stock PyTorch module supplied by the caller (``backbone=`` / ``backbones=``) or fetched by
``load_dinov2`` (torch.hub; unavailable offline).  A 4-D input ``[B, 3, H, W]`` (raw image batch,
uint8 or float) is first expanded on the GPU by the batched SWT kernel, so the model also accepts
what a deferred ``SWTTransform`` emits; the reference's 5-D ``[B, 3, 4, H, W]`` input is accepted
unchanged.
"""
import torch
import torch.nn as nn

from .. import _lib
from ..transforms import functional as TF
from .dsln import inject_domain_specific_layernorms
from .fusion import get_fusion_head


def load_dinov2(name, retries=1, **kwargs):
    """The reference's backbone loader (main/models/hub_utils.py:35-59): torch.hub, i.e. network or a populated hub
    cache.  Offline this raises; pass ``backbone=`` / ``backbones=`` to the model classes instead (the backbone is
    outside the accelerated path; bench and tests use wvhash.models.vit)."""
    last = None
    for _ in range(max(1, retries)):
        try:
            return torch.hub.load("facebookresearch/dinov2:main", name, skip_validation=True, **kwargs)
        except Exception as e:  # network / cache miss
            last = e
    raise RuntimeError(f"load_dinov2('{name}') failed ({type(last).__name__}: {last}): construct the model with "
                       "backbone=<nn.Module with .embed_dim> instead")


def hash_tail(fused, hash_fc, bn, want=("codes",), host_twin=False):
    """HIP tail: logits = hash_fc(fused); bn (eval); sign; pack.  -> dict of requested outputs.
    host_twin=True (explicit; never a silent fallback): host tensors take the library's host twin wv_hash_tail_cpu."""
    host = bool(host_twin) and not fused.is_cuda
    lib = _lib.load() if host else _lib.require_gpu()
    fused = fused.float().contiguous()
    B, E = fused.shape
    nbits = hash_fc.out_features
    dev = fused.device
    out = {}
    logits = torch.empty((B, nbits), dtype=torch.float32, device=dev) if "logits" in want else None
    codes = torch.empty((B, nbits), dtype=torch.float32, device=dev) if "codes" in want else None
    packed = torch.empty((B, (nbits + 63) // 64), dtype=torch.int64, device=dev) if "packed" in want else None
    use_bn = isinstance(bn, nn.BatchNorm1d)
    w = hash_fc.weight.detach().float().contiguous()
    hb = hash_fc.bias.detach().float().contiguous() if hash_fc.bias is not None else None
    bw = bn.weight.detach().float().contiguous() if use_bn else None
    bb = bn.bias.detach().float().contiguous() if use_bn else None
    bm = bn.running_mean.detach().float().contiguous() if use_bn else None
    bv = bn.running_var.detach().float().contiguous() if use_bn else None
    if B and host:
        rc = lib.wv_hash_tail_cpu(_lib.ptr(fused), B, E, _lib.ptr(w), _lib.ptr(hb), _lib.ptr(bw), _lib.ptr(bb), _lib.ptr(bm),
                                  _lib.ptr(bv), float(bn.eps) if use_bn else 0.0, nbits, _lib.ptr(logits), _lib.ptr(codes),
                                  _lib.ptr(packed))
        _lib.check(rc, "wv_hash_tail_cpu")
    elif B:
        with torch.cuda.device(dev):
            rc = lib.wv_hash_tail(_lib.ptr(fused), B, E, _lib.ptr(w), _lib.ptr(hb), _lib.ptr(bw), _lib.ptr(bb),
                                  _lib.ptr(bm), _lib.ptr(bv), float(bn.eps) if use_bn else 0.0, nbits,
                                  _lib.ptr(logits), _lib.ptr(codes), _lib.ptr(packed), _lib.stream_ptr())
            _lib.check(rc, "wv_hash_tail")
    out["logits"], out["codes"], out["packed"] = logits, codes, packed
    return out


def library_tail(module, features):
    """-> (take, host): whether hash_tail serves this call -- eval mode, no grad, GPU tensors or host tensors of a model with
    ``host_twin = True`` (explicit; never a silent fallback) -- and whether it is the host twin that does."""
    host = not features.is_cuda and getattr(module, "host_twin", False)
    take = not module.training and not torch.is_grad_enabled() and (features.is_cuda or host)
    return take, host


def freeze_backbone(module):
    """A frozen backbone: no gradients, eval mode, and it stays in eval mode when the model around it is put in train mode."""
    for p in module.parameters():
        p.requires_grad = False
    module.eval()
    module.train = lambda mode=False: None


def _cls(out):
    return out['x_norm_clstoken'] if isinstance(out, dict) else out


class _WaveletHashingBase(nn.Module):
    """Shared input handling.  The reference's models take the expanded ``[B, 3, 4, H, W]`` sub-band tensor
    (multi_dino_attention.py:815-818, :745); these take that unchanged, and also the raw ``[B, 3, H, W]`` image
    batch a deferred transform emits -- expanded here by the batched HIP kernel of the transform that was BOUND to
    the model (``bind_transform``; ``engine.evaluate`` binds ``dataset.transform`` by itself).  A raw batch carries
    no wavelet name, so without a bound transform a 4-D input is an error, never a default wavelet."""

    _bound_transform = None

    def bind_transform(self, transform):
        """``transform``: the wavelet plugin (or a pipeline / dataset holding one) that produced the raw batches."""
        from ..transforms.custom_transforms import find_wavelet_transform
        found = find_wavelet_transform(transform)
        if found is None:
            raise ValueError("bind_transform: no SWTTransform / RawStackTransform / DWTTransform in the given pipeline")
        self._bound_transform = found
        return self

    def set_wavelet(self, level=1, wavelet="haar"):
        """Shorthand: raw batches are to be expanded by SWTTransform(level, wavelet)."""
        from ..transforms import SWTTransform
        return self.bind_transform(SWTTransform(level=level, wavelet=wavelet, defer=True))

    def _raw_view(self, x):
        """-> (x, channels_last): a sizing.RawBatch (the collated batch of a sizing="device" pipeline) sized on the GPU --
        its images are [B, H, W, 3] -- and the [B,3,H,W] view of sized [B,H,W,3] images turned back, to be read in place."""
        from ..transforms.sizing import RawBatch
        if isinstance(x, RawBatch):
            return TF.size_images(x), True
        if x.dim() == 4 and x.shape[1] == 3 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous():
            return x.permute(0, 2, 3, 1), True
        return x, False

    def _transform_for_raw(self):
        if self._bound_transform is None:
            raise RuntimeError(
                "this model received a raw [B,3,H,W] image batch (a deferred transform's output) but no transform "
                "is bound to it: call model.bind_transform(dataset.transform) (wvhash.engine.evaluate does) or "
                "model.set_wavelet(level, wavelet); the wavelet is never guessed")
        return self._bound_transform

    @staticmethod
    def _band_dtype():
        """Under bf16 autocast the backbone's first op casts its input to bf16 anyway: the kernels emit bf16 directly."""
        bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        return torch.bfloat16 if bf16 else torch.float32

    def _band_major(self, x):
        """-> [4, B, 3, H, W] (band-major; a view whenever the memory already lies that way)."""
        x, channels_last = self._raw_view(x)
        if x.dim() == 5:
            return x.permute(2, 0, 1, 3, 4)
        if x.dim() != 4:
            raise ValueError(f"expected [B,3,4,H,W] sub-bands or a [B,3,H,W] image batch, got {tuple(x.shape)}")
        tf = self._transform_for_raw()
        from ..transforms import SWTTransform
        if isinstance(tf, SWTTransform):
            # written band-major by the kernel: the band split below is a view, the sub-bands exist once in HBM
            return TF.swt2d(x, tf.wavelet, tf.level, band_major=True, channels_last=channels_last,
                            out_dtype=self._band_dtype())
        return tf.apply_batch(x, channels_last=channels_last).permute(2, 0, 1, 3, 4)

    def _band(self, x, index, float_images=False):
        """-> [B, 3, H, W]: band `index` of the input, what a single-band model feeds its backbone.  A 5-D sub-band
        tensor gives the reference's view ``x[:, :, index]`` (detail_tester.py:36,100); a raw image batch goes through the
        bound transform's ``apply_band`` -- for SWTTransform the single-band kernel, which computes that band alone.
        ``float_images``: a float 4-D batch with no bound transform is already what the backbone reads (SingleBandNet's
        ``if x.dim() == 5``); a raw uint8 batch never is."""
        from ..transforms.sizing import RawBatch
        if not isinstance(x, RawBatch):
            if x.dim() == 5:
                return x[:, :, index]
            if x.dim() != 4:
                raise ValueError(f"expected [B,3,4,H,W] sub-bands or a [B,3,H,W] image batch, got {tuple(x.shape)}")
            if float_images and self._bound_transform is None and x.is_floating_point():
                return x
        tf = self._transform_for_raw()
        channels_last = False
        if not isinstance(x, RawBatch):          # apply_band sizes a RawBatch itself, as apply_batch does
            x, channels_last = self._raw_view(x)
        return tf.apply_band(x, index, channels_last=channels_last, out_dtype=self._band_dtype())

    def _tail(self, fused_embedding):
        take, host = library_tail(self, fused_embedding)
        if take:
            return hash_tail(fused_embedding, self.hash_fc, self.bn, want=("codes",), host_twin=host)["codes"]
        logits = self.bn(self.hash_fc(fused_embedding))
        return self._train_output(logits) if self.training else torch.sign(logits)

    def encode_packed(self, x):
        """Eval-mode forward that keeps the codes on the GPU as packed int64 words."""
        fused = self.fused_embedding(x)
        return hash_tail(fused, self.hash_fc, self.bn, want=("packed",))["packed"]


class SharedDinoHashing(_WaveletHashingBase):
    def __init__(self, backbone_config, fusion_config, binary_config, backbone=None, **kwargs):
        super().__init__()
        self.shared_backbone = backbone if backbone is not None else load_dinov2(backbone_config['name'])
        if backbone_config.get('frozen', True):
            freeze_backbone(self.shared_backbone)
        embed_dim = self.shared_backbone.embed_dim
        self.fusion_head = get_fusion_head(fusion_config, [embed_dim] * 4)
        self.nbits = binary_config['nbits']
        self.bn = nn.BatchNorm1d(self.nbits)
        self.hash_fc = nn.Linear(fusion_config['output_dim'], self.nbits, bias=False)
        nn.init.normal_(self.hash_fc.weight, std=0.01)

    def _train_output(self, logits):
        return torch.tanh(logits)

    def fused_embedding(self, x):
        bands = self._band_major(x)                      # [4, B, 3, H, W]
        s, b, c, h, w = bands.shape
        x_concat = bands.reshape(s * b, c, h, w)         # a view for kernel-written bands; the reference's copy
        cls_tokens = _cls(self.shared_backbone(x_concat))  # (multi_dino_attention.py:818) for a 5-D input
        return self.fusion_head(list(cls_tokens.chunk(4, dim=0)))

    def forward(self, x):
        return self._tail(self.fused_embedding(x))


class MultiDinoHashing(_WaveletHashingBase):
    def __init__(self, backbones_config, fusion_config, binary_config, use_bn=True, backbones=None, **kwargs):
        super().__init__()
        self.backbones = nn.ModuleList()
        output_dims = []
        for i, bb_cfg in enumerate(backbones_config):
            model = backbones[i] if backbones is not None else load_dinov2(bb_cfg['name'])
            if bb_cfg.get('frozen', True):
                freeze_backbone(model)
            self.backbones.append(model)
            output_dims.append(model.embed_dim)
        self.fusion_head = get_fusion_head(fusion_config, output_dims)
        self.nbits = binary_config['nbits']
        self.use_bn = use_bn
        self.bn = nn.BatchNorm1d(self.nbits) if use_bn else nn.Identity()
        self.hash_fc = nn.Linear(fusion_config['output_dim'], self.nbits, bias=not use_bn)
        nn.init.normal_(self.hash_fc.weight, std=0.01)
        if not use_bn:
            nn.init.zeros_(self.hash_fc.bias)

    def _train_output(self, logits):
        return logits

    def fused_embedding(self, x):
        bands = self._band_major(x)                      # bands[i] = x[..., i, :, :] (:745)
        features = [_cls(backbone(bands[i])) for i, backbone in enumerate(self.backbones)]
        return self.fusion_head(features)

    def forward(self, x):
        return self._tail(self.fused_embedding(x))


class PromptedSharedDinoHashing(_WaveletHashingBase):
    """The prompt-tuned shared backbone (multi_dino_attention.py:835-899): ``num_prompts`` learned tokens per band between
    the CLS token and the patch tokens.  ``backbone_config['use_dsln']`` swaps every LayerNorm of the backbone for a
    MultiDomainLayerNorm (one LayerNorm per band); without gradients those run the grouped LayerNorm kernel, and the block
    norms -- whose only readers are the qkv / fc1 Linears -- emit bf16 under bf16 autocast (``emit_dtype = "auto"``).  The
    final norm keeps the stock dtype: the fusion head reads it."""

    def __init__(self, backbone_config, fusion_config, binary_config, num_prompts=10, backbone=None, **kwargs):
        super().__init__()
        self.shared_backbone = backbone if backbone is not None else load_dinov2(backbone_config['name'])
        self.use_dsln = backbone_config.get('use_dsln', False)
        if self.use_dsln:
            self.shared_backbone = inject_domain_specific_layernorms(self.shared_backbone, num_domains=4)
            for blk in self.shared_backbone.blocks:
                blk.norm1.emit_dtype = blk.norm2.emit_dtype = "auto"
        if backbone_config.get('frozen', True):
            freeze_backbone(self.shared_backbone)
        embed_dim = self.shared_backbone.embed_dim
        self.num_prompts = num_prompts
        self.prompts = nn.Parameter(torch.randn(4, num_prompts, embed_dim) * 0.02)
        self.fusion_head = get_fusion_head(fusion_config, [embed_dim] * 4)
        self.nbits = binary_config['nbits']
        self.bn = nn.BatchNorm1d(self.nbits)
        self.hash_fc = nn.Linear(fusion_config['output_dim'], self.nbits, bias=False)
        nn.init.normal_(self.hash_fc.weight, std=0.01)

    def _train_output(self, logits):
        return torch.tanh(logits)

    def fused_embedding(self, x):
        bands = self._band_major(x)                      # [4, B, 3, H, W]
        s, b, c, h, w = bands.shape
        x_tokens = self.shared_backbone.prepare_tokens_with_masks(bands.reshape(s * b, c, h, w))
        prompts = self.prompts.unsqueeze(1).expand(-1, b, -1, -1).reshape(s * b, self.num_prompts, -1)
        tokens = torch.cat([x_tokens[:, 0:1, :], prompts, x_tokens[:, 1:, :]], dim=1)
        for blk in self.shared_backbone.blocks:
            tokens = blk(tokens)
        tokens = self.shared_backbone.norm(tokens)
        return self.fusion_head(list(tokens[:, 0].chunk(4, dim=0)))

    def forward(self, x):
        return self._tail(self.fused_embedding(x))
