from .fusion import (CrossAttentionBottleneckHead, CrossAttentionBottleneckHeadAdvanced,
                     CrossAttentionBottleneckHeadPooled, CrossAttentionBottleneckHeadDecoupled,
                     get_fusion_head, band_attn_pool, band_attn_maps, BandMultiheadAttention)
from .fusion_extra import (AdvancedFusionModule, AttentionFusionHead, GatedFusionHead, SemanticFusionHead, StandardFusionHead,
                           TemperatureFusionHead, TemperatureGatedFusionHead)
from .dsln import MultiDomainLayerNorm, inject_domain_specific_layernorms, group_layernorm
from .hashing import SharedDinoHashing, MultiDinoHashing, PromptedSharedDinoHashing, hash_tail, load_dinov2
from .single_band import SingleBandNet, DINOHashBaseline, DetailTesterNet

__all__ = ["CrossAttentionBottleneckHead", "CrossAttentionBottleneckHeadAdvanced",
           "CrossAttentionBottleneckHeadPooled", "CrossAttentionBottleneckHeadDecoupled", "get_fusion_head",
           "band_attn_pool", "band_attn_maps", "BandMultiheadAttention", "SharedDinoHashing", "MultiDinoHashing", "hash_tail", "load_dinov2", "StandardFusionHead",
           "TemperatureFusionHead", "SemanticFusionHead", "GatedFusionHead", "TemperatureGatedFusionHead",
           "AttentionFusionHead", "AdvancedFusionModule", "SingleBandNet", "DINOHashBaseline", "DetailTesterNet",
           "PromptedSharedDinoHashing", "MultiDomainLayerNorm", "inject_domain_specific_layernorms", "group_layernorm"]
