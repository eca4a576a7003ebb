"""Shared by tests/golden/make_golden_prompted.py and the prompted-model tests: the seeded stand-in for the DINOv2 backbone
(wvhash.models.vit.tiny_vit restated: 2 blocks, 384 wide, 14-pixel patches, DINOv2's module names and its
``prepare_tokens_with_masks``), the fixture's cases, the shared input and the exemption rule for code bits.

A full state dict of one case is about 20 MB, far above what a committed fixture may hold.  The fixture therefore stores the
state dict as its keys, shapes and a SHA-256 over all values; both sides fill the model with wvhash.synth.randomize_module
under the case's seed -- every parameter and buffer, sorted by name, from one generator -- and the tests check keys, shapes
and digest before they compare outputs.  The small tensors (BatchNorm, the final norm) are stored verbatim as well.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

EMBED = 384
IMG = 28                                  # 2 x 2 patches of 14 pixels: 1 + num_prompts + 4 tokens
INPUT_SHAPE = (5, 3, 4, IMG, IMG)         # B = 5: 4 B = 20 sequences
EXEMPT_FACTOR = 16.0                      # code bits with |reference logit| <= 16 * d64 are not compared
EXEMPT_CAP = 0.02                         # ... and the maker refuses a fixture with more than 2 % of them

FUSION = {"use_all_tokens": False, "type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "dropout": 0.0,
          "num_queries": 4, "sub_band_dropout_p": 0, "ortho_weight": 0.01}

# name -> (use_dsln, num_prompts, frozen, construction seed, state seed)
CASES = {
    "dsln_p10": (True, 10, False, 201, 301),
    "dsln_p1": (True, 1, False, 202, 302),
    "plain_p10": (False, 10, False, 203, 303),
    "plain_p1_frozen": (False, 1, True, 204, 304),
}
# the bare MultiDomainLayerNorm on sequence counts that 4 domains do not divide: name -> (N, T, E, state seed)
BARE_CASES = {"bare_n6": (6, 5, 96, 401), "bare_n3": (3, 5, 96, 402), "bare_n10": (10, 2, 96, 403)}


def model_kwargs(name):
    use_dsln, num_prompts, frozen, _, _ = CASES[name]
    return dict(backbone_config={"name": "dinov2_vits14", "frozen": frozen, "use_dsln": use_dsln}, fusion_config=dict(FUSION),
                binary_config={"nbits": 64}, num_prompts=num_prompts)


class _Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        x = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class _LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(1e-5 * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, heads)
        self.ls1 = _LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim)
        self.ls2 = _LayerScale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class _PatchEmbed(nn.Module):
    def __init__(self, patch, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class TinyViT(nn.Module):
    """Module names, construction order (so: RNG consumption) and forward of wvhash.models.vit.tiny_vit(384, img_size=28)."""

    def __init__(self, embed_dim=EMBED, depth=2, num_heads=6, patch_size=14, img_size=IMG):
        super().__init__()
        self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        n = (img_size // patch_size) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.randn(1, n + 1, embed_dim) * 0.02)
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)

    def prepare_tokens_with_masks(self, x, masks=None):
        x = self.patch_embed(x)
        return torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self.pos_embed

    def forward(self, x):
        x = self.prepare_tokens_with_masks(x)
        for blk in self.blocks:
            x = blk(x)
        x = self.norm(x)
        return {"x_norm_clstoken": x[:, 0], "x_norm_patchtokens": x[:, 1:]}


def make_input():
    return torch.randn(*INPUT_SHAPE, generator=torch.Generator().manual_seed(2025))


def bare_input(name):
    N, T, E, seed = BARE_CASES[name]
    return torch.randn(N, T, E, generator=torch.Generator().manual_seed(seed + 50)) * 2 + 1


def state_layout(module):
    """Keys and shapes of the state dict, as the fixture stores them."""
    sd = module.state_dict()
    keys = sorted(sd)
    return np.array(keys), np.array([",".join(str(d) for d in sd[k].shape) for k in keys])


def small_state(module):
    """The tensors the fixture stores verbatim: BatchNorm and the backbone's final norm."""
    return {k: v.detach().clone() for k, v in module.state_dict().items()
            if k.startswith("bn.") or k.startswith("shared_backbone.norm.")}


def exempt_mask(ref_logits, d):
    """True where a code bit is NOT compared: the reference logit lies within EXEMPT_FACTOR * d of zero, d = how far the
    reference's own fp32 logits are from the same model in float64 (two fp32 orders of evaluation differ by about as much)."""
    return ref_logits.abs() <= EXEMPT_FACTOR * d


class LogitTap(object):
    """Forward hook on ``bn``: keeps its last output (the logits whose sign is the code)."""

    def __init__(self, model):
        self.logits = None
        self.handle = model.bn.register_forward_hook(self._keep)

    def _keep(self, module, args, output):
        self.logits = output.detach()

    def close(self):
        self.handle.remove()
