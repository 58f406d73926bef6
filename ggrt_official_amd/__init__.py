"""ggrt_official_amd — MI355X-native differentiable 3D-Gaussian rasterizer, drop-in for the
``diff_gaussian_rasterization`` extension GGRt uses on its render hot path
(reference ``ggrt/model/pixelsplat/decoder/cuda_splatting.py``).

Scope: the rasterizer (forward + backward) behind a C ABI, the call-site glue
(`render_cuda`, `render_depth_cuda`, `DecoderSplattingCUDA`), one-frame-per-GPU sharding helpers and a
synthetic-scene generator for the benchmark.  Everything else of GGRt is out of scope.
"""
from .rasterizer import (Contributions, GaussianRasterizationSettings, GaussianRasterizer, PixelHits, PixelPicks, Projection, clear_list_hints,
                         composite_hits, last_forward_status, list_hint_stats, pick_values, rasterize_gaussians, rasterize_views,
                         set_list_hint, sort_watch_stats)
from .splatting import (DepthHead, EpipolarSamples, FusedConvGRU, FusedSepConvGRU, ImageLoss, PhotometricLoss, epipolar_attention_core,
                        epipolar_encoded_attention_core, fused_depth_head, fused_epipolar_attention, fused_epipolar_encoded_attention,
                        fused_epipolar_sampler, fused_gaussian_adapter, fused_gru_half, fused_gru_half_inference, fused_image_loss, fused_photometric_loss, fused_ssim,
                        fused_upsample_depth, fused_warp_cost, gru_blend, gru_conv, gru_gate)

__all__ = ["Contributions", "PixelPicks", "pick_values", "PixelHits", "composite_hits", "Projection", "GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians",
           "rasterize_views", "fused_gaussian_adapter", "fused_depth_head", "DepthHead", "fused_epipolar_sampler", "EpipolarSamples",
           "fused_epipolar_attention", "epipolar_attention_core", "fused_epipolar_encoded_attention", "epipolar_encoded_attention_core",
           "fused_image_loss", "fused_ssim", "ImageLoss", "fused_photometric_loss", "PhotometricLoss", "fused_warp_cost", "fused_upsample_depth",
           "gru_gate", "gru_blend", "fused_gru_half", "fused_gru_half_inference", "gru_conv", "FusedSepConvGRU", "FusedConvGRU",
           "last_forward_status", "set_list_hint", "list_hint_stats", "clear_list_hints", "sort_watch_stats"]
__version__ = "0.1.0"
