"""Shared by tests/golden/make_golden_single_band.py and the single-band model tests: the tiny stand-in for the DINOv2
backbone (embed_dim = 384, dict output like the hub model), the fixture's cases and its key layout."""
import numpy as np
import torch
import torch.nn as nn

EMBED = 384
INPUT_SHAPE = (5, 3, 4, 16, 16)

# name -> (class name, constructor kwargs)
CASES = {
    "sb_hash_bn_d1": ("SingleBandNet", dict(detail_index=1, output_dim=64, is_hashing=True, use_bn=True)),
    "sb_hash_nobn_d2": ("SingleBandNet", dict(detail_index=2, output_dim=64, is_hashing=True, use_bn=False)),
    "sb_embed_d0": ("SingleBandNet", dict(detail_index=0, output_dim=384, is_hashing=False, use_bn=True)),
    "sb_embed_proj_d3": ("SingleBandNet", dict(detail_index=3, output_dim=32, is_hashing=False, use_bn=False)),
    "dino_baseline": ("DINOHashBaseline", dict(dino_backbone="dinov2_vits14", embed_dim=384, binary_config={"nbits": 64})),
    "detail_tester_d1": ("DetailTesterNet", dict(backbone_name="dinov2_vits14", detail_index=1, output_dim=64)),
}


class TinyBackbone(nn.Module):
    """[B, 3, H, W] -> {'x_norm_clstoken': [B, 384]}: 2 x 2 average pooling and one Linear."""

    def __init__(self, seed=0):
        super().__init__()
        self.embed_dim = EMBED
        self.pool = nn.AdaptiveAvgPool2d(2)
        self.proj = nn.Linear(12, EMBED)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(EMBED, 12, generator=g))
            self.proj.bias.copy_(0.1 * torch.randn(EMBED, generator=g))

    def forward(self, x):
        return {"x_norm_clstoken": self.proj(self.pool(x).flatten(1))}


def model_input(name, x5):
    """What the case's model is fed: the sub-band tensor, or (DINOHashBaseline) a plain image batch."""
    return x5[:, :, 0].contiguous() if CASES[name][0] == "DINOHashBaseline" else x5


def load_state(npz, name):
    prefix = f"{name}/state/"
    return {k[len(prefix):]: torch.from_numpy(np.asarray(npz[k])) for k in npz.files if k.startswith(prefix)}
