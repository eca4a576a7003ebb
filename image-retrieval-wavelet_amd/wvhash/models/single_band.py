"""The single-band and baseline hashing models of the reference's ablation and control arms: class names, kwargs and
state_dict keys of /root/reference/main/models/detail_tester.py (SingleBandNet :55-114, DetailTesterNet :7-51) and
main/models/dino_baseline.py (DINOHashBaseline).

What runs where:
* the band a single-band model reads -- ``x[:, :, detail_index]`` of the sub-band tensor -- comes, for a raw image batch
  (a deferred transform's output), from the bound transform's ``apply_band``: for SWTTransform the single-band HIP kernel
  (wv_swt2d_band_forward), which neither computes nor writes the other three bands;
* the DINOv2 backbone is a stock PyTorch module (``backbone=`` or ``load_dinov2``);
* the eval-mode hashing tails of SingleBandNet (``is_hashing``) and DINOHashBaseline -- Linear -> BatchNorm1d -> sign
  [-> pack] -- are the HIP tail ``hash_tail`` (wv_hash_tail; its host twin with ``model.host_twin = True``);
* DetailTesterNet's tail is BatchNorm1d BEFORE the Linear, not the order wv_hash_tail implements: stock PyTorch;
* training, and eval under grad, are stock PyTorch everywhere.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .hashing import _WaveletHashingBase, _cls, freeze_backbone, hash_tail, library_tail, load_dinov2


class SingleBandNet(_WaveletHashingBase):
    """One DINOv2 ViT-S/14 on one SWT sub-band (detail_tester.py:55-114).  ``backbone_name`` and the other YAML keys of
    config/model/single_band.yaml are swallowed, as in the reference: the backbone is dinov2_vits14 unless injected."""

    def __init__(self, detail_index=0, output_dim=384, is_hashing=False, use_bn=True, backbone=None, **kwargs):
        super().__init__()
        self.detail_index = detail_index
        self.is_hashing = is_hashing
        self.use_bn = use_bn if is_hashing else False
        self.backbone = backbone if backbone is not None else load_dinov2('dinov2_vits14')
        embed_dim = self.backbone.embed_dim
        if output_dim == embed_dim and not is_hashing:
            self.head = nn.Identity()
        else:
            self.head = nn.Linear(embed_dim, output_dim, bias=not self.use_bn)
            nn.init.normal_(self.head.weight, std=0.01)
            if self.head.bias is not None:
                nn.init.constant_(self.head.bias, 0)
        self.bn = nn.BatchNorm1d(output_dim) if self.use_bn else nn.Identity()

    def features(self, x):
        return _cls(self.backbone(self._band(x, self.detail_index, float_images=True)))

    def forward(self, x):
        features = self.features(x)
        if not self.is_hashing:
            return F.normalize(self.head(features), p=2, dim=1)
        take, host = library_tail(self, features)
        if take:
            return hash_tail(features, self.head, self.bn, want=("codes",), host_twin=host)["codes"]
        out = self.bn(self.head(features))
        return out if self.training else torch.sign(out)      # raw logits in training: HashLoss applies the tanh

    def encode_packed(self, x):
        """Eval-mode forward that keeps the codes on the GPU as packed int64 words."""
        if not self.is_hashing:
            raise RuntimeError("encode_packed: this SingleBandNet was built with is_hashing=False (it emits embeddings)")
        return hash_tail(self.features(x), self.head, self.bn, want=("packed",))["packed"]


class DINOHashBaseline(nn.Module):
    """DINOv2 + Linear(no bias) -> BatchNorm1d on plain [B, 3, H, W] images (dino_baseline.py): no wavelet involved."""

    def __init__(self, dino_backbone='dinov2_vits14', embed_dim=384, binary_config={'nbits': 64}, frozen=False,
                 backbone=None, **kwargs):
        super().__init__()
        self.backbone = backbone if backbone is not None else load_dinov2(dino_backbone)
        self.frozen = frozen
        if frozen:
            freeze_backbone(self.backbone)
        self.hash_head = nn.Sequential(
            nn.Linear(embed_dim, binary_config['nbits'], bias=False),
            nn.BatchNorm1d(binary_config['nbits'])
        )

    def features(self, x):
        # never re-enables grad inside an outer no_grad block; a frozen backbone builds no graph
        with torch.set_grad_enabled(torch.is_grad_enabled() and not self.frozen):
            return _cls(self.backbone(x))

    def forward(self, x):
        features = self.features(x)
        take, host = library_tail(self, features)
        if take:
            return hash_tail(features, self.hash_head[0], self.hash_head[1], want=("codes",), host_twin=host)["codes"]
        logits = self.hash_head(features)
        return logits if self.training else torch.sign(logits)

    def encode_packed(self, x):
        """Eval-mode forward that keeps the codes on the GPU as packed int64 words."""
        return hash_tail(self.features(x), self.hash_head[0], self.hash_head[1], want=("packed",))["packed"]


class DetailTesterNet(_WaveletHashingBase):
    """One backbone on one SWT sub-band, BatchNorm1d(dim) -> Linear(dim, output_dim) -> tanh / sign
    (detail_tester.py:7-51).  Only the dinov2 branch exists here; the tail is stock PyTorch (see the module text)."""

    def __init__(self, backbone_name='resnet50', detail_index=1, output_dim=64, backbone=None, **kwargs):
        super().__init__()
        if 'dinov2' not in backbone_name:
            raise ValueError(f"DetailTesterNet: backbone_name={backbone_name!r}: timm backbones (ResNet, ConvNeXt) are "
                             "outside this library; only the dinov2 branch of the reference is built")
        self.detail_index = detail_index
        self.backbone = backbone if backbone is not None else load_dinov2(backbone_name)
        dim = self.backbone.embed_dim
        self.pool = nn.Identity()
        self.bn = nn.BatchNorm1d(dim)
        self.hash_fc = nn.Linear(dim, output_dim)
        nn.init.normal_(self.hash_fc.weight, std=0.01)
        nn.init.constant_(self.hash_fc.bias, 0)

    def forward(self, x):
        feat = _cls(self.backbone(self._band(x, self.detail_index)))
        logits = self.hash_fc(self.bn(feat))
        return torch.tanh(logits) if self.training else torch.sign(logits)
