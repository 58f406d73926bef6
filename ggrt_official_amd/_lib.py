"""ctypes binding of the C ABI declared in ``include/ggr_raster.h``.

There is deliberately NO fallback: if ``libggr_raster.so`` is missing or does not export the
symbols the header declares, importing the rasterizer raises.  (The CPU restatements under
``oracle/`` are test infrastructure and are never reachable from here.)
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libggr_raster.so")
ABI_VERSION = 11

c_float_p = C.c_void_p  # device pointers travel as integers


class GgrSettings(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32), ("sh_degree", C.c_int32),
        ("sh_stride", C.c_int32), ("num_points", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("scale_modifier", C.c_float), ("bg", C.c_void_p), ("viewmatrix", C.c_void_p),
        ("projmatrix", C.c_void_p), ("campos", C.c_void_p), ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("tanfov_dev", C.c_void_p), ("sh_max_degree", C.c_int32), ("scissor", C.c_int32 * 4), ("reference_rects", C.c_int32),
        ("depth_sort", C.c_int32),
    ]


class GgrForwardIn(C.Structure):
    _fields_ = [
        ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p), ("opacities", C.c_void_p),
        ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("aux_precomp", C.c_void_p),
        ("input_scale", C.c_void_p), ("cov3D_full", C.c_int32), ("sh_channel_major", C.c_int32),
        ("aux_affine", C.c_int32), ("aux_a", C.c_float), ("aux_b", C.c_float),
    ]


class GgrViews(C.Structure):
    _fields_ = [
        ("num_views", C.c_int32), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
        ("bg", C.c_void_p), ("tanfov", C.c_void_p), ("input_scale", C.c_void_p), ("num_sets", C.c_int32),
    ]


class GgrForwardOut(C.Structure):
    _fields_ = [
        ("out_color", C.c_void_p), ("radii", C.c_void_p), ("out_depth", C.c_void_p), ("geom_buffer", C.c_void_p),
        ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
        ("stage_ms", C.c_void_p), ("binning_capacity", C.c_int64), ("no_backward", C.c_int32),
        ("backward_scratch", C.c_void_p), ("capacity_is_hint", C.c_int32), ("max_list_len", C.c_int32),
        ("depth_sort_used", C.c_int32),
    ]


class GgrBackwardIn(C.Structure):
    _fields_ = [
        ("fwd", GgrForwardIn), ("radii", C.c_void_p), ("geom_buffer", C.c_void_p), ("image_buffer", C.c_void_p),
        ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64), ("dL_dout_color", C.c_void_p),
        ("dL_dout_depth", C.c_void_p), ("scratch", C.c_void_p), ("scratch_zeroed", C.c_int32),
    ]


class GgrBackwardOut(C.Structure):
    _fields_ = [
        ("dL_dmeans3D", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_dshs", C.c_void_p),
        ("dL_dcolors_precomp", C.c_void_p), ("dL_dopacities", C.c_void_p), ("dL_dcov3D", C.c_void_p),
        ("dL_dscales", C.c_void_p), ("dL_drotations", C.c_void_p), ("dL_daux", C.c_void_p),
        ("dL_dviewmatrix", C.c_void_p),
        ("dL_dprojmatrix", C.c_void_p), ("dL_dcampos", C.c_void_p), ("stage_ms", C.c_void_p),
    ]

class GgrForwardOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("antialiasing", C.c_int32)]


def forward_options(antialiasing: bool = False) -> GgrForwardOptions:
    """The options of ggr_forward_opt / ggr_forward_views_opt (include/ggr_raster.h), struct_size filled in."""
    return GgrForwardOptions(struct_size=C.sizeof(GgrForwardOptions), antialiasing=int(bool(antialiasing)))


class GgrForwardExtra(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("out_alpha", C.c_void_p)]


class GgrBackwardExtra(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("dL_dout_alpha", C.c_void_p)]


class GgrBackwardExtra2(C.Structure):
    """GgrBackwardExtra with dL_dtanfov behind it: the `_ext` backward calls take either, struct_size tells which."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("dL_dout_alpha", C.c_void_p),
                ("dL_dtanfov", C.c_void_p)]


def forward_extra(out_alpha=None) -> GgrForwardExtra:
    """The extra planes of ggr_forward_ext / ggr_forward_views_ext (include/ggr_raster.h), struct_size filled in."""
    return GgrForwardExtra(struct_size=C.sizeof(GgrForwardExtra), reserved=0, out_alpha=out_alpha)


def backward_extra(dL_dout_alpha=None) -> GgrBackwardExtra:
    """The extra planes of ggr_backward_ext / ggr_backward_views_ext, struct_size filled in."""
    return GgrBackwardExtra(struct_size=C.sizeof(GgrBackwardExtra), reserved=0, dL_dout_alpha=dL_dout_alpha)


def backward_extra2(dL_dout_alpha=None, dL_dtanfov=None):
    """A GgrBackwardExtra2 (struct_size filled in) as the `extra` argument of ggr_backward_ext / ggr_backward_views_ext:
    returns (pointer for the call, the struct — keep it alive across the call)."""
    ex = GgrBackwardExtra2(struct_size=C.sizeof(GgrBackwardExtra2), reserved=0, dL_dout_alpha=dL_dout_alpha,
                           dL_dtanfov=dL_dtanfov)
    return C.cast(C.pointer(ex), C.POINTER(GgrBackwardExtra)), ex


MAX_FEATURES = 32   # GGR_MAX_FEATURES


class GgrFeaturePass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_features", C.c_int32), ("features", C.c_void_p),
                ("geom_buffer", C.c_void_p), ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p),
                ("num_rendered", C.c_int64), ("out_features", C.c_void_p), ("dL_dout_features", C.c_void_p),
                ("dL_dfeatures", C.c_void_p), ("scratch", C.c_void_p), ("scratch_zeroed", C.c_int32),
                ("reserved", C.c_int32)]


def feature_pass(**fields) -> GgrFeaturePass:
    """The argument of ggr_features_forward / ggr_features_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrFeaturePass(struct_size=C.sizeof(GgrFeaturePass), **fields)


class GgrContributionPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("out_weight_sum", C.c_void_p), ("out_weight_max", C.c_void_p), ("out_pixel_count", C.c_void_p)]


def contribution_pass(**fields) -> GgrContributionPass:
    """The argument of ggr_contributions (include/ggr_raster.h), struct_size filled in."""
    return GgrContributionPass(struct_size=C.sizeof(GgrContributionPass), **fields)


class GgrPickPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("out_median_index", C.c_void_p), ("out_median_depth", C.c_void_p), ("out_max_index", C.c_void_p),
                ("out_max_weight", C.c_void_p), ("out_count", C.c_void_p)]


def pick_pass(**fields) -> GgrPickPass:
    """The argument of ggr_pixel_picks (include/ggr_raster.h), struct_size filled in."""
    return GgrPickPass(struct_size=C.sizeof(GgrPickPass), **fields)


MAX_HITS = 32   # GGR_MAX_HITS


class GgrHitPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_hits", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("out_index", C.c_void_p), ("out_weight", C.c_void_p), ("out_rest", C.c_void_p), ("out_count", C.c_void_p)]


def hit_pass(**fields) -> GgrHitPass:
    """The argument of ggr_pixel_hits (include/ggr_raster.h), struct_size filled in."""
    return GgrHitPass(struct_size=C.sizeof(GgrHitPass), **fields)


class GgrHitGradPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_hits", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("weight", C.c_void_p), ("rest", C.c_void_p), ("count", C.c_void_p), ("dL_dweight", C.c_void_p),
                ("dL_drest", C.c_void_p), ("scratch", C.c_void_p), ("scratch_zeroed", C.c_int32), ("reserved", C.c_int32)]


def hit_grad_pass(**fields) -> GgrHitGradPass:
    """The argument of ggr_pixel_hits_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrHitGradPass(struct_size=C.sizeof(GgrHitGradPass), **fields)


class GgrProjectionPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("geom_buffer", C.c_void_p), ("radii", C.c_void_p),
                ("out_means2d", C.c_void_p), ("out_depth", C.c_void_p), ("out_conic", C.c_void_p), ("out_opacity", C.c_void_p),
                ("out_color", C.c_void_p), ("out_valid", C.c_void_p), ("dL_dmeans2d", C.c_void_p), ("dL_ddepth", C.c_void_p),
                ("dL_dconic", C.c_void_p), ("dL_dopacity", C.c_void_p), ("dL_dcolor", C.c_void_p), ("scratch", C.c_void_p),
                ("scratch_zeroed", C.c_int32), ("reserved2", C.c_int32)]


def projection_pass(**fields) -> GgrProjectionPass:
    """The argument of ggr_projection / ggr_projection_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrProjectionPass(struct_size=C.sizeof(GgrProjectionPass), **fields)


class GgrAdapterPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("num_cameras", C.c_int32), ("gaussians_per_camera", C.c_int32),
                ("samples_per_row", C.c_int32), ("d_sh", C.c_int32), ("scale_min", C.c_float), ("scale_max", C.c_float),
                ("eps", C.c_float), ("debug", C.c_int32), ("reserved2", C.c_int32), ("reserved3", C.c_int32),
                ("depth", C.c_void_p), ("coords", C.c_void_p), ("raw", C.c_void_p), ("c2w", C.c_void_p), ("Kinv", C.c_void_p),
                ("q_cam", C.c_void_p), ("scale_mult", C.c_void_p), ("sh_transform", C.c_void_p), ("sh_mask", C.c_void_p),
                ("out_means", C.c_void_p), ("out_scales", C.c_void_p), ("out_quats", C.c_void_p), ("out_harmonics", C.c_void_p),
                ("dL_dmeans", C.c_void_p), ("dL_dscales", C.c_void_p), ("dL_dquats", C.c_void_p), ("dL_dharmonics", C.c_void_p),
                ("dL_draw", C.c_void_p), ("dL_ddepth", C.c_void_p), ("dL_dcoords", C.c_void_p), ("dL_dc2w", C.c_void_p),
                ("dL_dKinv", C.c_void_p), ("dL_dq_cam", C.c_void_p), ("dL_dscale_mult", C.c_void_p), ("dL_dsh_transform", C.c_void_p)]


def adapter_pass(**fields) -> GgrAdapterPass:
    """The argument of ggr_adapter_forward / ggr_adapter_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrAdapterPass(struct_size=C.sizeof(GgrAdapterPass), **fields)


class GgrDepthHeadPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("num_cameras", C.c_int32), ("rays_per_camera", C.c_int32),
                ("num_buckets", C.c_int32), ("num_surfaces", C.c_int32), ("samples_per_ray", C.c_int32), ("deterministic", C.c_int32),
                ("use_transmittance", C.c_int32), ("xy_raw_stride", C.c_int32), ("debug", C.c_int32), ("reserved2", C.c_int32),
                ("opacity_exponent", C.c_float), ("opacity_scale", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float),
                ("logits", C.c_void_p), ("xy_raw", C.c_void_p), ("ray_xy", C.c_void_p), ("near", C.c_void_p), ("far", C.c_void_p),
                ("u", C.c_void_p), ("out_depth", C.c_void_p), ("out_opacity", C.c_void_p), ("out_coords", C.c_void_p),
                ("index", C.c_void_p), ("dL_ddepth", C.c_void_p), ("dL_dopacity", C.c_void_p), ("dL_dcoords", C.c_void_p),
                ("dL_dlogits", C.c_void_p), ("dL_dxy_raw", C.c_void_p)]


def depth_head_pass(**fields) -> GgrDepthHeadPass:
    """The argument of ggr_depth_head_forward / ggr_depth_head_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrDepthHeadPass(struct_size=C.sizeof(GgrDepthHeadPass), **fields)


class GgrEpipolarPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int32), ("num_views", C.c_int32),
                ("channels", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("num_samples", C.c_int32),
                ("use_window", C.c_int32), ("window_y0", C.c_int32), ("window_y1", C.c_int32), ("window_x0", C.c_int32),
                ("window_x1", C.c_int32), ("debug", C.c_int32), ("image_strides", C.c_int64 * 5),
                ("c2w", C.c_void_p), ("w2c", C.c_void_p), ("K", C.c_void_p), ("Kinv", C.c_void_p), ("near", C.c_void_p),
                ("far", C.c_void_p), ("images", C.c_void_p), ("features", C.c_void_p), ("valid", C.c_void_p), ("xy_ray", C.c_void_p),
                ("xy_sample", C.c_void_p), ("xy_sample_near", C.c_void_p), ("xy_sample_far", C.c_void_p), ("origins", C.c_void_p),
                ("directions", C.c_void_p), ("depth", C.c_void_p), ("segment", C.c_void_p), ("dL_dfeatures", C.c_void_p),
                ("dL_dimages", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


def epipolar_pass(**fields) -> GgrEpipolarPass:
    """The argument of ggr_epipolar_forward / ggr_epipolar_backward (include/ggr_raster.h), struct_size filled in;
    `image_strides` may be any sequence of five integers."""
    if "image_strides" in fields:
        fields["image_strides"] = (C.c_int64 * 5)(*fields["image_strides"])
    return GgrEpipolarPass(struct_size=C.sizeof(GgrEpipolarPass), **fields)


class GgrEpipolarAttnPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("N", C.c_int32), ("S", C.c_int32), ("C", C.c_int32),
                ("H", C.c_int32), ("qk", C.c_void_p), ("z", C.c_void_p), ("out_ctx", C.c_void_p), ("out_attn", C.c_void_p),
                ("attn", C.c_void_p), ("dL_dctx", C.c_void_p), ("dL_dqk", C.c_void_p), ("dL_dz", C.c_void_p)]


def epipolar_attn_pass(**fields) -> GgrEpipolarAttnPass:
    """The argument of ggr_epipolar_attention_forward / _backward (include/ggr_raster.h), struct_size filled in."""
    return GgrEpipolarAttnPass(struct_size=C.sizeof(GgrEpipolarAttnPass), **fields)


class GgrEpipolarAttnEncPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("N", C.c_int32), ("S", C.c_int32), ("C", C.c_int32),
                ("H", C.c_int32), ("num_octaves", C.c_int32), ("reserved2", C.c_int32), ("qk", C.c_void_p), ("qe", C.c_void_p),
                ("features", C.c_void_p), ("depth", C.c_void_p), ("out_ctx_f", C.c_void_p), ("out_ctx_e", C.c_void_p),
                ("out_attn", C.c_void_p), ("attn", C.c_void_p), ("dL_dctx_f", C.c_void_p), ("dL_dctx_e", C.c_void_p),
                ("dL_dqk", C.c_void_p), ("dL_dqe", C.c_void_p), ("dL_dfeatures", C.c_void_p), ("dL_ddepth", C.c_void_p)]


def epipolar_attn_enc_pass(**fields) -> GgrEpipolarAttnEncPass:
    """The argument of ggr_epipolar_attention_encoded_forward / _backward (include/ggr_raster.h), struct_size filled in."""
    return GgrEpipolarAttnEncPass(struct_size=C.sizeof(GgrEpipolarAttnEncPass), **fields)


class GgrImageLossPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int32), ("channels", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("window_size", C.c_int32), ("size_average", C.c_int32),
                ("pred", C.c_void_p), ("target", C.c_void_p), ("mask", C.c_void_p), ("out_mse", C.c_void_p), ("out_ssim", C.c_void_p),
                ("mse_scale", C.c_void_p), ("partials", C.c_void_p), ("partials_bytes", C.c_int64), ("dL_dmse", C.c_void_p),
                ("dL_dssim", C.c_void_p), ("dL_dpred", C.c_void_p), ("dL_dtarget", C.c_void_p)]


def image_loss_pass(**fields) -> GgrImageLossPass:
    """The argument of ggr_image_loss_forward / ggr_image_loss_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrImageLossPass(struct_size=C.sizeof(GgrImageLossPass), **fields)


class GgrPhotometricLossPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("num_views", C.c_int32), ("num_iters", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("automask", C.c_int32), ("reserved2", C.c_int32),
                ("ssim_loss_weight", C.c_float), ("smooth_loss_weight", C.c_float), ("C1", C.c_float), ("C2", C.c_float),
                ("clip_loss", C.c_float), ("gamma", C.c_float), ("image", C.c_void_p), ("ref_imgs", C.c_void_p),
                ("inv_depths", C.c_void_p), ("K", C.c_void_p), ("ref_Ks", C.c_void_p), ("poses", C.c_void_p), ("planes", C.c_void_p),
                ("planes_bytes", C.c_int64), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out_thresholds", C.c_void_p),
                ("state", C.c_void_p), ("choice", C.c_void_p), ("out_loss", C.c_void_p), ("out_photometric", C.c_void_p),
                ("out_smoothness", C.c_void_p), ("dL_dloss", C.c_void_p), ("dL_dinv_depths", C.c_void_p), ("dL_dposes", C.c_void_p)]


def photometric_loss_pass(**fields) -> GgrPhotometricLossPass:
    """The argument of ggr_photometric_loss_forward / _backward (include/ggr_raster.h), struct_size filled in."""
    return GgrPhotometricLossPass(struct_size=C.sizeof(GgrPhotometricLossPass), **fields)


class GgrWarpCostPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("num_views", C.c_int32), ("channels", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("reduce_mean", C.c_int32), ("fold_disp", C.c_int32),
                ("scale_factor", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float), ("reserved2", C.c_int32),
                ("fmap", C.c_void_p), ("fmaps_ref", C.c_void_p), ("inv_depth", C.c_void_p), ("K", C.c_void_p), ("ref_Ks", C.c_void_p),
                ("poses", C.c_void_p), ("out_cost", C.c_void_p), ("out_cells", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("dL_dcost", C.c_void_p), ("dL_dfmap", C.c_void_p), ("dL_dfmaps_ref", C.c_void_p),
                ("dL_dinv_depth", C.c_void_p), ("dL_dposes", C.c_void_p)]


def warp_cost_pass(**fields) -> GgrWarpCostPass:
    """The argument of ggr_warp_cost_forward / _backward (include/ggr_raster.h), struct_size filled in."""
    return GgrWarpCostPass(struct_size=C.sizeof(GgrWarpCostPass), **fields)


class GgrUpsampleDepthPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("ratio", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32), ("fold_disp", C.c_int32), ("reserved2", C.c_int32),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("depth", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("dL_dout", C.c_void_p), ("dL_dmask", C.c_void_p),
                ("dL_ddepth", C.c_void_p)]


def upsample_depth_pass(**fields) -> GgrUpsampleDepthPass:
    """The argument of ggr_upsample_depth_forward / _backward (include/ggr_raster.h), struct_size filled in."""
    return GgrUpsampleDepthPass(struct_size=C.sizeof(GgrUpsampleDepthPass), **fields)


class GgrGruPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32)] + [(f, C.c_void_p) for f in (
                    "a_zr_h", "a_zr_x", "h", "z", "r", "rh", "a_q_h", "a_q_x", "q", "out_h", "dL_dout_h", "dL_da_q", "dL_da_zr", "dL_dh_part",
                    "dL_drh", "dL_dh")]


def gru_pass(**fields) -> GgrGruPass:
    """The argument of ggr_gru_gate_forward / _blend_forward / _blend_backward / _gate_backward (include/ggr_raster.h), struct_size
    filled in."""
    return GgrGruPass(struct_size=C.sizeof(GgrGruPass), **fields)


class GgrGruConvPass(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("struct_size", "reserved", "batch", "channels", "in_channels", "height", "width", "kernel_h", "kernel_w",
                                         "epilogue", "out_channels")] + [(f, C.c_void_p) for f in (
                    "a", "x", "w_h", "w_x", "bias", "h", "z", "rh", "out_h", "raw", "workspace")] + [("workspace_bytes", C.c_int64)]


GRU_CONV_GATE, GRU_CONV_BLEND, GRU_CONV_RAW = 0, 1, 2


def gru_conv_pass(**fields) -> GgrGruConvPass:
    """The argument of ggr_gru_conv_forward / ggr_gru_conv_workspace_bytes (include/ggr_raster.h), struct_size filled in."""
    return GgrGruConvPass(struct_size=C.sizeof(GgrGruConvPass), **fields)


class GgrDistortionPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("out_distortion", C.c_void_p), ("totals", C.c_void_p), ("dL_dout_distortion", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_zeroed", C.c_int32), ("reserved2", C.c_int32)]


def distortion_pass(**fields) -> GgrDistortionPass:
    """The argument of ggr_distortion_forward / ggr_distortion_backward (include/ggr_raster.h), struct_size filled in."""
    return GgrDistortionPass(struct_size=C.sizeof(GgrDistortionPass), **fields)


class GgrAbsgradPass(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("geom_buffer", C.c_void_p),
                ("image_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("num_rendered", C.c_int64),
                ("out_color", C.c_void_p), ("out_depth", C.c_void_p), ("dL_dout_color", C.c_void_p),
                ("dL_dout_depth", C.c_void_p), ("dL_dout_alpha", C.c_void_p), ("out_absgrad", C.c_void_p),
                ("out_grad", C.c_void_p)]


def absgrad_pass(**fields) -> GgrAbsgradPass:
    """The argument of ggr_means2d_absgrad (include/ggr_raster.h), struct_size filled in."""
    return GgrAbsgradPass(struct_size=C.sizeof(GgrAbsgradPass), **fields)


FWD_STAGES = ["preprocess", "depth_sort", "tile_count", "tile_scatter", "blend", "colour_side_stream", "tile_sort"]
DEPTH_SORT = {"auto": 0, "global": 1, "per_tile": 2, "global_3pass": 0x101}
DEPTH_SORT_NO_BUCKETS = 0x100      # IN flag: never the global sort's bucket form (include/ggr_raster.h)
DEPTH_SORT_FELL_BACK = 0x201       # OUT: the bucket form gave a frame up; its lists were built again in three passes
DEPTH_SORT_SLOW = 0x401            # OUT: the bucket form built the lists, the slow way (depths concentrated: include/ggr_raster.h)
BWD_STAGES = ["clear", "blend", "preprocess"]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

# every symbol include/ggr_raster.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("ggr_abi_version", C.c_int, []),
    ("ggr_last_error", C.c_char_p, []),
    ("ggr_source_hash", C.c_char_p, []),
    ("ggr_geom_bytes", C.c_size_t, [C.c_int32]),
    ("ggr_image_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ggr_binning_bytes", C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    ("ggr_work_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_backward_scratch_bytes", C.c_size_t, [C.c_int32]),
    ("ggr_forward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrForwardIn), C.POINTER(GgrForwardOut),
                              ALLOC_FN, C.c_void_p, C.c_void_p]),
    ("ggr_backward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrBackwardIn), C.POINTER(GgrBackwardOut),
                               C.c_void_p]),
    ("ggr_image_bytes_inference", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_geom_bytes_inference", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ggr_geom_bytes_views", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ggr_image_bytes_views", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_work_bytes_views", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_backward_scratch_bytes_views", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ggr_forward_views", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrForwardIn),
                                    C.POINTER(GgrForwardOut), ALLOC_FN, C.c_void_p, C.c_void_p]),
    ("ggr_backward_views", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrBackwardIn),
                                     C.POINTER(GgrBackwardOut), C.c_void_p]),
    ("ggr_forward_opt", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrForwardOptions), C.POINTER(GgrForwardIn),
                                  C.POINTER(GgrForwardOut), ALLOC_FN, C.c_void_p, C.c_void_p]),
    ("ggr_forward_views_opt", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrForwardOptions), C.POINTER(GgrViews),
                                        C.POINTER(GgrForwardIn), C.POINTER(GgrForwardOut), ALLOC_FN, C.c_void_p,
                                        C.c_void_p]),
    ("ggr_forward_ext", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrForwardOptions), C.POINTER(GgrForwardExtra),
                                  C.POINTER(GgrForwardIn), C.POINTER(GgrForwardOut), ALLOC_FN, C.c_void_p, C.c_void_p]),
    ("ggr_backward_ext", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrBackwardExtra), C.POINTER(GgrBackwardIn),
                                   C.POINTER(GgrBackwardOut), C.c_void_p]),
    ("ggr_forward_views_ext", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrForwardOptions), C.POINTER(GgrForwardExtra),
                                        C.POINTER(GgrViews), C.POINTER(GgrForwardIn), C.POINTER(GgrForwardOut), ALLOC_FN,
                                        C.c_void_p, C.c_void_p]),
    ("ggr_backward_views_ext", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrBackwardExtra), C.POINTER(GgrViews),
                                         C.POINTER(GgrBackwardIn), C.POINTER(GgrBackwardOut), C.c_void_p]),
    ("ggr_features_forward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrFeaturePass), C.c_void_p]),
    ("ggr_features_backward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrFeaturePass), C.c_void_p]),
    ("ggr_contributions", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrContributionPass), C.c_void_p]),
    ("ggr_pixel_picks", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrPickPass), C.c_void_p]),
    ("ggr_pixel_hits", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrHitPass), C.c_void_p]),
    ("ggr_pixel_hits_backward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrHitGradPass), C.c_void_p]),
    ("ggr_projection", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrProjectionPass), C.c_void_p]),
    ("ggr_projection_backward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrProjectionPass), C.c_void_p]),
    ("ggr_adapter_forward", C.c_int, [C.POINTER(GgrAdapterPass), C.c_void_p]),
    ("ggr_adapter_backward", C.c_int, [C.POINTER(GgrAdapterPass), C.c_void_p]),
    ("ggr_depth_head_forward", C.c_int, [C.POINTER(GgrDepthHeadPass), C.c_void_p]),
    ("ggr_depth_head_backward", C.c_int, [C.POINTER(GgrDepthHeadPass), C.c_void_p]),
    ("ggr_epipolar_scratch_bytes", C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_epipolar_forward", C.c_int, [C.POINTER(GgrEpipolarPass), C.c_void_p]),
    ("ggr_epipolar_backward", C.c_int, [C.POINTER(GgrEpipolarPass), C.c_void_p]),
    ("ggr_epipolar_attention_forward", C.c_int, [C.POINTER(GgrEpipolarAttnPass), C.c_void_p]),
    ("ggr_epipolar_attention_backward", C.c_int, [C.POINTER(GgrEpipolarAttnPass), C.c_void_p]),
    ("ggr_epipolar_attention_encoded_forward", C.c_int, [C.POINTER(GgrEpipolarAttnEncPass), C.c_void_p]),
    ("ggr_epipolar_attention_encoded_backward", C.c_int, [C.POINTER(GgrEpipolarAttnEncPass), C.c_void_p]),
    ("ggr_image_loss_partials_bytes", C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("ggr_image_loss_window", C.c_int, [C.c_int32, C.POINTER(C.c_float)]),
    ("ggr_image_loss_forward", C.c_int, [C.POINTER(GgrImageLossPass), C.c_void_p]),
    ("ggr_image_loss_backward", C.c_int, [C.POINTER(GgrImageLossPass), C.c_void_p]),
    ("ggr_photometric_loss_planes_bytes", C.c_int64, [C.c_int32] * 5),
    ("ggr_photometric_loss_workspace_bytes", C.c_int64, [C.c_int32] * 5),
    ("ggr_photometric_loss_forward", C.c_int, [C.POINTER(GgrPhotometricLossPass), C.c_void_p]),
    ("ggr_photometric_loss_backward", C.c_int, [C.POINTER(GgrPhotometricLossPass), C.c_void_p]),
    ("ggr_warp_cost_workspace_bytes", C.c_int64, [C.c_int32] * 3),
    ("ggr_warp_cost_forward", C.c_int, [C.POINTER(GgrWarpCostPass), C.c_void_p]),
    ("ggr_warp_cost_backward", C.c_int, [C.POINTER(GgrWarpCostPass), C.c_void_p]),
    ("ggr_upsample_depth_workspace_bytes", C.c_int64, [C.c_int32] * 4),
    ("ggr_upsample_depth_forward", C.c_int, [C.POINTER(GgrUpsampleDepthPass), C.c_void_p]),
    ("ggr_upsample_depth_backward", C.c_int, [C.POINTER(GgrUpsampleDepthPass), C.c_void_p]),
    ("ggr_gru_gate_forward", C.c_int, [C.POINTER(GgrGruPass), C.c_void_p]),
    ("ggr_gru_blend_forward", C.c_int, [C.POINTER(GgrGruPass), C.c_void_p]),
    ("ggr_gru_blend_backward", C.c_int, [C.POINTER(GgrGruPass), C.c_void_p]),
    ("ggr_gru_gate_backward", C.c_int, [C.POINTER(GgrGruPass), C.c_void_p]),
    ("ggr_gru_conv_workspace_bytes", C.c_size_t, [C.POINTER(GgrGruConvPass)]),
    ("ggr_gru_conv_forward", C.c_int, [C.POINTER(GgrGruConvPass), C.c_void_p]),
    ("ggr_distortion_forward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrDistortionPass), C.c_void_p]),
    ("ggr_distortion_backward", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrDistortionPass), C.c_void_p]),
    ("ggr_means2d_absgrad", C.c_int, [C.POINTER(GgrSettings), C.POINTER(GgrViews), C.POINTER(GgrAbsgradPass), C.c_void_p]),
    ("ggr_camera_setup", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ggr_camera_setup_backward", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ggr_forward_status", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p]),
    ("ggr_sort_stats_async", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ggr_mark_visible", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ggr_debug_readback_wait", C.c_int, [C.c_int32, C.c_double, C.POINTER(C.c_uint32)]),
    ("ggr_debug_counters", C.c_int, [C.POINTER(C.c_uint64), C.c_int32]),
    ("ggr_debug_host_slots", C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("ggr_debug_copy", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    ("ggr_debug_unpack_geom", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ggr_debug_unpack_binning", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
]

_lib = None


def load():
    """dlopen the HIP library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f"{LIB_PATH} does not export {name}")
        fn.restype = restype
        fn.argtypes = argtypes
    v = lib.ggr_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {v}, binding expects {ABI_VERSION}")
    # the library must have been built from the csrc/ tree next to it (a stale .so would otherwise be what gets tested
    # and measured).  GGR_SKIP_SOURCE_HASH=1: dev builds only (scripts/build_variants.sh ships several libraries).
    if os.environ.get("GGR_SKIP_SOURCE_HASH", "0") != "1":
        from . import _build
        built = lib.ggr_source_hash().decode("ascii", "replace")
        try:
            want = _build.source_hash()
        except FileNotFoundError:   # a binary-only installation (no csrc/ next to the library): nothing to compare with
            want = built
        if built != want:
            raise ImportError(
                f"{LIB_PATH} was built from other sources than {_build.CSRC} holds now (library {built[:12]}…, tree "
                f"{want[:12]}…): run `python __graft_entry__.py build`. There is no CPU fallback.")
    _lib = lib
    return lib


def last_error() -> str:
    return load().ggr_last_error().decode("utf-8", "replace")
