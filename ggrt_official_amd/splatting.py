"""Call-site layer: what GGRt wraps around the rasterizer.

Mirrors, with the same names / argument meaning / results, the reference's
``ggrt/model/pixelsplat/decoder/cuda_splatting.py`` (``get_projection_matrix`` :18-46,
``render_cuda`` :49-128, ``render_depth_cuda`` :227-269) and
``decoder/decoder_splatting_cuda.py`` (``DecoderSplattingCUDA`` :19-85), so that GGRt's ``PixelSplat``
(``pixelsplat.py:144,230``) can use this module unchanged.  Written from the behaviour of those
functions (pinned by the golden vectors under ``tests/golden/``), not from their text:
no einops / jaxtyping, all per-view quantities computed batched, no ``.item()`` syncs in the loop
(``tan(fov/2)`` is derived on the host side once for the whole batch).

Reference quirks kept on purpose (drop-in parity):
  * the projection matrix uses ``intrinsics[0]`` for EVERY batch element (``cuda_splatting.py:39-42``);
  * ``scale_invariant`` divides translations / means by ``near`` and covariances by ``near²`` (:66-73);
  * the depth pass feeds depth as a degree-0 SH coefficient, so the rasterizer returns
    ``0.5 + C0·z`` per channel and the result is the channel mean (:256-269);
  * ``sh_degree = isqrt(d_sh) - 1`` (GGRt: d_sh = 25 → 4); bands 0..min(sh_degree, cap) are evaluated.  The cap is
    per call (``sh_max_degree=`` of every function here; ``DecoderSplattingCUDA(sh_max_degree=…)`` per INSTANCE) and
    otherwise this layer's default ``SH_MAX_DEGREE`` (``set_sh_max_degree`` / ``GGR_SH_MAX_DEGREE``) — the default the
    ``diff_gaussian_rasterization`` import shim uses too, so that GGRt's own ``cuda_splatting.py`` on the shim and this
    module render one checkpoint identically (``tests/test_gpu_one_checkpoint_one_answer.py``).  The default
    is 4 for THIS layer unless chosen otherwise: the package GGRt's README installs is
    pixelSplat's rasterizer fork, GGRt's encoder emits, masks and Wigner-rotates all of bands 0..4
    (``encoder/common/gaussian_adapter.py:45-46,90``) and passes ``sh_degree = 4`` on purpose; 3 reproduces the
    graphdeco / w-depth family (coefficients 16.. ignored); the raw ``GaussianRasterizer`` keeps "not chosen → 3 with
    one warning".  What the choice moves on a GGRt-like scene is measured in INTEGRATION.md §7.
"""
from __future__ import annotations

import itertools
import os
from dataclasses import dataclass
from math import isqrt
from typing import Literal, NamedTuple, Optional

import ctypes as C

import torch
from torch import Tensor, nn

from . import _lib
from .rasterizer import Contributions, GaussianRasterizationSettings, GaussianRasterizer, PixelHits, PixelPicks, Projection

DepthRenderingMode = Literal["depth", "disparity", "relative_disparity", "log"]

# Highest SH band the rasterizer evaluates for this call site (GaussianRasterizationSettings.sh_max_degree).
# 4 (this layer's default): band 4 is evaluated and differentiated when the call passes sh_degree >= 4
# with >= 25 coefficients, as GGRt does; 3: coefficients 16.. are ignored (graphdeco / w-depth family); 0 hands the
# decision to the raw rasterizer ("not chosen": 3, with one warning the first time coefficients 16.. go unused).
SH_MAX_DEGREE = int(os.environ.get("GGR_SH_MAX_DEGREE", "4") or 4)


def set_sh_max_degree(cap: int) -> int:
    """Chooses the DEFAULT (process-wide: this call-site layer and the ``diff_gaussian_rasterization`` import shim) for the
    highest SH band the rasterizer evaluates: 3 or 4 (0 = leave it to the raw rasterizer: "not chosen", 3 with one warning).
    A per-call / per-instance ``sh_max_degree`` takes precedence.  Returns the previous setting."""
    global SH_MAX_DEGREE
    if int(cap) not in (0, 3, 4):
        raise ValueError("sh_max_degree must be 3 or 4")
    prev, SH_MAX_DEGREE = SH_MAX_DEGREE, int(cap)
    return prev


def resolve_sh_max_degree(cap: Optional[int] = None) -> int:
    """The cap a call uses: its own explicit choice, else this layer's default as it is NOW."""
    if cap is None:
        return SH_MAX_DEGREE
    if int(cap) not in (0, 3, 4):
        raise ValueError("sh_max_degree must be 3 or 4")
    return int(cap)


@dataclass
class Gaussians:
    """Same fields as reference ``ggrt/model/pixelsplat/types.py:7-12``."""
    means: Tensor        # [b, g, 3]
    covariances: Tensor  # [b, g, 3, 3]
    harmonics: Tensor    # [b, g, 3, d_sh]
    opacities: Tensor    # [b, g]
    # fused-adapter form (§8f-4): set ``covariances=None`` and give the ellipsoids as world-space
    # (scales, (w,x,y,z) quaternions) from ``adapter_scale_rotation``
    scales: Optional[Tensor] = None     # [b, g, 3]
    rotations: Optional[Tensor] = None  # [b, g, 4]


@dataclass
class DecoderOutput:
    color: Tensor            # [b, v, 3, h, w]
    depth: Optional[Tensor]  # [b, v, h, w]
    alpha: Optional[Tensor] = None  # [b, v, h, w]: accumulated opacity 1 − T (DecoderSplattingCUDA(..., return_alpha=True))
    features: Optional[Tensor] = None  # [b, v, K, h, w]: Σ f·α·T of the per-Gaussian channels (…, gaussian_features=[b,g,K])
    contributions: Optional[Contributions] = None  # [b, v, g] tensors: Σ w, max w, pixel count (…, return_contributions=True)
    picks: Optional[PixelPicks] = None  # [b, v, h, w] planes: median depth / index, dominant weight / index, count (…, return_picks=True)
    hits: Optional[PixelHits] = None  # index / weight [b, v, K, h, w], rest / count [b, v, h, w]: the first K composited Gaussians (…, return_hits=K)
    projection: Optional[Projection] = None  # [b, v, g, …] rows: 2D mean, depth value, conic, opacity, colour, valid (…, return_projection=True)


def get_fov(intrinsics: Tensor) -> Tensor:
    """[b,3,3] normalised intrinsics → [b,2] (fov_x, fov_y): angle between the rays through the
    mid-points of opposite image edges (reference ``ggrt/geometry/projection.py:233-247``)."""
    inv = torch.linalg.inv(intrinsics)

    def ray(u, v):
        p = torch.tensor([u, v, 1.0], dtype=torch.float32, device=intrinsics.device)
        d = inv @ p
        return d / d.norm(dim=-1, keepdim=True)

    fov_x = (ray(0.0, 0.5) * ray(1.0, 0.5)).sum(-1).acos()
    fov_y = (ray(0.5, 0.0) * ray(0.5, 1.0)).sum(-1).acos()
    return torch.stack((fov_x, fov_y), dim=-1)


def get_projection_matrix(near: Tensor, far: Tensor, fov_x: Tensor, fov_y: Tensor, intrinsics: Tensor) -> Tensor:
    """GGRt-modified perspective matrix [b,4,4] (reference ``cuda_splatting.py:18-46``): X/Y → (-1,1)
    with an off-centre principal point, Z → (0,1).  ``fov_*`` are accepted for signature parity but,
    as in the reference, only ``intrinsics[0]`` determines the X/Y rows."""
    b = near.shape[0]
    P = torch.zeros((b, 4, 4), dtype=torch.float32, device=near.device)
    k0 = intrinsics[0]
    P[:, 0, 0] = 2 * near * k0[0, 0]
    P[:, 1, 1] = 2 * near * k0[1, 1]
    P[:, 0, 2] = 2 * k0[0, 2] - 1
    P[:, 1, 2] = 2 * k0[1, 2] - 1
    P[:, 3, 2] = 1
    P[:, 2, 2] = far / (far - near)
    P[:, 2, 3] = -(far * near) / (far - near)
    return P


_TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def quaternion_to_matrix(q_xyzw: Tensor, eps: float = 1e-8) -> Tensor:
    """(x,y,z,w) quaternions (any norm) → rotation matrices (reference ``encoder/common/gaussians.py:8-31``)."""
    i, j, k, r = q_xyzw.unbind(-1)
    s = 2 / ((q_xyzw * q_xyzw).sum(-1) + eps)
    m = torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                     s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1)
    return m.reshape(*q_xyzw.shape[:-1], 3, 3)


def adapter_covariances(scales: Tensor, rotations_xyzw: Tensor, c2w_rotations: Tensor) -> Tensor:
    """World-space covariance the way the reference's adapter builds it: ``C·R·S·Sᵀ·Rᵀ·Cᵀ``
    (``encoder/common/gaussians.py:33-44`` + ``gaussian_adapter.py:79-81``) → [...,3,3]."""
    L = c2w_rotations @ quaternion_to_matrix(rotations_xyzw) * scales[..., None, :]
    return L @ L.transpose(-1, -2)


def matrix_to_quaternion_wxyz(m: Tensor) -> Tensor:
    """Rotation matrices [...,3,3] → unit (w,x,y,z); picks the best-conditioned of the four branches."""
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    cand = torch.stack([
        torch.stack([1 + m00 + m11 + m22, m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]], -1),
        torch.stack([m[..., 2, 1] - m[..., 1, 2], 1 + m00 - m11 - m22, m[..., 0, 1] + m[..., 1, 0], m[..., 0, 2] + m[..., 2, 0]], -1),
        torch.stack([m[..., 0, 2] - m[..., 2, 0], m[..., 0, 1] + m[..., 1, 0], 1 - m00 + m11 - m22, m[..., 1, 2] + m[..., 2, 1]], -1),
        torch.stack([m[..., 1, 0] - m[..., 0, 1], m[..., 0, 2] + m[..., 2, 0], m[..., 1, 2] + m[..., 2, 1], 1 - m00 - m11 + m22], -1),
    ], -2)
    pick = torch.stack([m00 + m11 + m22, m00, m11, m22], -1).argmax(-1)
    q = torch.gather(cand, -2, pick[..., None, None].expand(*pick.shape, 1, 4)).squeeze(-2)
    return q / q.norm(dim=-1, keepdim=True)


def adapter_scale_rotation(scales: Tensor, rotations_xyzw: Tensor, c2w_rotations: Tensor, eps: float = 1e-8):
    """what the rasterizer needs INSTEAD of ``adapter_covariances`` — the same ellipsoid as
    (scales[...,3], world-space unit quaternion (w,x,y,z)[...,4]), 28 B per Gaussian instead of a 36-B matrix
    plus the [.,3,3] temporaries of three batched matmuls.  The camera-to-world rotation is composed onto
    the Gaussian's quaternion (Hamilton product); ``R S Sᵀ Rᵀ`` itself is then evaluated inside the HIP
    preprocess kernel (``scales``/``rotations`` inputs) and differentiated by its backward."""
    qc = matrix_to_quaternion_wxyz(c2w_rotations)
    x, y, z, w = (rotations_xyzw / (rotations_xyzw.norm(dim=-1, keepdim=True) + eps)).unbind(-1)
    cw, cx, cy, cz = qc.unbind(-1)
    q = torch.stack([cw * w - cx * x - cy * y - cz * z,
                     cw * x + cx * w + cy * z - cz * y,
                     cw * y - cx * z + cy * w + cz * x,
                     cw * z + cx * y - cy * x + cz * w], -1)
    return scales.broadcast_to(q.shape[:-1] + (3,)), q


def adapter_sh_mask(d_sh: int, device=None) -> Tensor:
    """The reference adapter's harmonics mask [d_sh]: 1 for the DC term, ``0.1·0.25^degree`` for every higher band
    (``gaussian_adapter.py:39-46``)."""
    mask = torch.ones(d_sh, dtype=torch.float32, device=device)
    for degree in range(1, isqrt(d_sh)):
        mask[degree ** 2:(degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return mask


class _FusedAdapter(torch.autograd.Function):
    """ggr_adapter_forward / ggr_adapter_backward (csrc/adapter.hip) behind autograd: the per-Gaussian tensors and the tiny
    per-camera tensors in, (means, scales, quats wxyz, harmonics) out — one launch each way."""

    @staticmethod
    def forward(ctx, depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask, scale_min, scale_max, eps):
        dev = depth.device
        if dev.type != "cuda":
            raise RuntimeError("fused_gaussian_adapter runs on the GPU only (there is no CPU fallback)")
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask = map(f, (depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask))
        n_cam, g = depth.shape
        d_sh = sh_t.shape[-1]
        rows = raw.shape[1]
        if rows < 1 or g % rows != 0 or raw.shape != (n_cam, rows, 7 + 3 * d_sh):
            raise ValueError(f"raw_gaussians {tuple(raw.shape)} does not fit {n_cam} cameras x {g} Gaussians with d_sh = {d_sh}")
        ctx.dims = (n_cam, g, g // rows, d_sh, float(scale_min), float(scale_max), float(eps))
        p = n_cam * g
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        means, scales, quats, harmonics = new(p, 3), new(p, 3), new(p, 4), new(p, 3, d_sh)
        ap = _FusedAdapter._pass(ctx.dims, depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask, out_means=means.data_ptr(),
                                 out_scales=scales.data_ptr(), out_quats=quats.data_ptr(), out_harmonics=harmonics.data_ptr())
        with torch.cuda.device(dev):
            rc = _lib.load().ggr_adapter_forward(C.byref(ap), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"ggr_adapter_forward failed (code {rc}): {_lib.last_error()}")
        ctx.save_for_backward(depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask)
        return means, scales, quats, harmonics

    @staticmethod
    def _pass(dims, depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, sh_mask, **more):
        n_cam, g, spp, d_sh, scale_min, scale_max, eps = dims
        return _lib.adapter_pass(reserved=0, num_cameras=n_cam, gaussians_per_camera=g, samples_per_row=spp, d_sh=d_sh,
                                 scale_min=scale_min, scale_max=scale_max, eps=eps, debug=0, reserved2=0, reserved3=0,
                                 depth=depth.data_ptr(), coords=coords.data_ptr(), raw=raw.data_ptr(), c2w=c2w.data_ptr(),
                                 Kinv=kinv.data_ptr(), q_cam=q_cam.data_ptr(), scale_mult=mult.data_ptr(),
                                 sh_transform=sh_t.data_ptr(), sh_mask=sh_mask.data_ptr(), **more)

    @staticmethod
    def backward(ctx, g_means, g_scales, g_quats, g_harm):
        saved = ctx.saved_tensors
        depth, coords, raw, c2w, kinv, q_cam, mult, sh_t, _ = saved
        dev = depth.device
        f = lambda t: t.to(dtype=torch.float32).contiguous()
        g_means, g_scales, g_quats, g_harm = map(f, (g_means, g_scales, g_quats, g_harm))
        need = ctx.needs_input_grad
        d_raw = torch.empty_like(raw)
        d_depth = torch.empty_like(depth) if need[0] else None
        d_coords = torch.empty_like(coords) if need[1] else None
        # the per-camera sums are added into: zero-initialised here, NULL (skipped by the kernel) where nobody asks
        d_c2w, d_kinv, d_q, d_mult, d_sh_t = (torch.zeros_like(t) if need[i] else None
                                              for i, t in ((3, c2w), (4, kinv), (5, q_cam), (6, mult), (7, sh_t)))
        ptr = lambda t: None if t is None else t.data_ptr()
        ap = _FusedAdapter._pass(ctx.dims, *saved, dL_dmeans=g_means.data_ptr(), dL_dscales=g_scales.data_ptr(),
                                 dL_dquats=g_quats.data_ptr(), dL_dharmonics=g_harm.data_ptr(), dL_draw=d_raw.data_ptr(),
                                 dL_ddepth=ptr(d_depth), dL_dcoords=ptr(d_coords), dL_dc2w=ptr(d_c2w), dL_dKinv=ptr(d_kinv),
                                 dL_dq_cam=ptr(d_q), dL_dscale_mult=ptr(d_mult), dL_dsh_transform=ptr(d_sh_t))
        with torch.cuda.device(dev):
            rc = _lib.load().ggr_adapter_backward(C.byref(ap), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"ggr_adapter_backward failed (code {rc}): {_lib.last_error()}")
        return (d_depth, d_coords, d_raw if need[2] else None, d_c2w, d_kinv, d_q, d_mult, d_sh_t, None, None, None, None)


def fused_gaussian_adapter(extrinsics: Tensor, intrinsics: Tensor, coordinates: Tensor, depths: Tensor, raw_gaussians: Tensor,
                           image_shape, sh_transform: Tensor, *, scale_min: float, scale_max: float,
                           sh_mask: Optional[Tensor] = None, eps: float = 1e-8) -> Gaussians:
    """GGRt's ``GaussianAdapter.forward`` (``encoder/common/gaussian_adapter.py:48-96``) as one HIP launch, and one more for its
    backward.  C source cameras of G Gaussians each: ``extrinsics`` [C,4,4] camera-to-world, ``intrinsics``
    [C,3,3] normalised, ``coordinates`` [C,G,2], ``depths`` [C,G], ``raw_gaussians`` [C,G/spp,7+3·d_sh] (scale logits 3,
    quaternion xyzw 4, harmonics ``(xyz d_sh)``; spp consecutive Gaussians share a row — the reference's broadcast sample axis),
    ``sh_transform`` [C,d_sh,d_sh]: the caller's Wigner-D matrices of the cameras' rotations, of which the diagonal band blocks are
    read.  ``sh_mask=None``: the reference's (``adapter_sh_mask``).  Returns ``Gaussians`` with P = C·G rows in the form the
    boundary takes unchanged: ``covariances=None``, world-space ``scales`` [P,3] and ``rotations`` [P,4] (w,x,y,z) as
    ``adapter_scale_rotation`` gives them, ``harmonics`` [P,3,d_sh]; ``opacities=None`` (not the adapter's business).
    The per-camera quantities are derived here in torch with autograd on, so gradients reach ``extrinsics``, ``intrinsics`` and
    ``sh_transform`` through torch's own backward of those tiny ops; the kernels see no Gaussian-sized torch op."""
    d_sh = sh_transform.shape[-1]
    if d_sh not in (1, 4, 9, 16, 25) or sh_transform.shape[-2] != d_sh:
        raise ValueError("sh_transform must be [C, d_sh, d_sh] with d_sh in {1, 4, 9, 16, 25}")
    h, w = image_shape
    dev = depths.device
    if sh_mask is None:
        sh_mask = adapter_sh_mask(d_sh, dev)
    pixel_size = torch.tensor([1.0 / w, 1.0 / h], dtype=intrinsics.dtype, device=intrinsics.device)
    mult = 0.1 * (torch.linalg.inv(intrinsics[..., :2, :2]) @ pixel_size).sum(-1)     # get_scale_multiplier
    means, scales, quats, harmonics = _FusedAdapter.apply(
        depths, coordinates, raw_gaussians, extrinsics[..., :3, :4], torch.linalg.inv(intrinsics),
        matrix_to_quaternion_wxyz(extrinsics[..., :3, :3]), mult, sh_transform, sh_mask, scale_min, scale_max, eps)
    return Gaussians(means=means, covariances=None, harmonics=harmonics, opacities=None, scales=scales, rotations=quats)


@dataclass
class DepthHead:
    """What ``fused_depth_head`` returns, per Gaussian p = c·G + (r·srf + j)·spp + k: the adapter's and the decoder's inputs."""
    depths: Tensor         # [C, G]
    opacities: Tensor      # [C, G]
    coordinates: Tensor    # [C, G, 2]
    index: Tensor          # [C, G] int32: the chosen depth bucket (no gradient)


# tests only: True fills every buffer the depth-head launches must write whole with NaN (index: -1) before the launch
_DEPTH_HEAD_POISON = False


def _depth_head_buffer(shape, dtype, dev):
    if _DEPTH_HEAD_POISON:
        return torch.full(shape, -1 if dtype == torch.int32 else float("nan"), dtype=dtype, device=dev)
    return torch.empty(shape, dtype=dtype, device=dev)


class _FusedDepthHead(torch.autograd.Function):
    """ggr_depth_head_forward / ggr_depth_head_backward (csrc/depth_head.hip) behind autograd: one launch each way.  `xy_raw` arrives
    as [C, R·srf, 2] with a unit inner stride and one common row stride (read in place)."""

    @staticmethod
    def forward(ctx, logits, xy_raw, ray_xy, near, far, u, dims):
        dev = logits.device
        n_cam, rays, s, srf, spp, deterministic, transmittance, exponent, scale, inv_w, inv_h = dims
        g = rays * srf * spp
        depth, opacity = _depth_head_buffer((n_cam, g), torch.float32, dev), _depth_head_buffer((n_cam, g), torch.float32, dev)
        coords, index = _depth_head_buffer((n_cam, g, 2), torch.float32, dev), _depth_head_buffer((n_cam, g), torch.int32, dev)
        ctx.dims = dims
        ctx.set_materialize_grads(False)     # (an output nobody used arrives as None and goes to the launch as NULL)
        dp = _FusedDepthHead._pass(dims, logits, xy_raw, ray_xy, near, far, index, u=None if u is None else u.data_ptr(),
                                   out_depth=depth.data_ptr(), out_opacity=opacity.data_ptr(), out_coords=coords.data_ptr())
        with torch.cuda.device(dev):
            rc = _lib.load().ggr_depth_head_forward(C.byref(dp), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"ggr_depth_head_forward failed (code {rc}): {_lib.last_error()}")
        ctx.save_for_backward(logits, xy_raw, ray_xy, near, far, index)
        ctx.mark_non_differentiable(index)
        return depth, opacity, coords, index

    @staticmethod
    def _pass(dims, logits, xy_raw, ray_xy, near, far, index, **more):
        n_cam, rays, s, srf, spp, deterministic, transmittance, exponent, scale, inv_w, inv_h = dims
        stride = xy_raw.stride(1) if xy_raw.shape[1] > 1 else max(2, xy_raw.stride(1))
        return _lib.depth_head_pass(reserved=0, num_cameras=n_cam, rays_per_camera=rays, num_buckets=s, num_surfaces=srf,
                                    samples_per_ray=spp, deterministic=int(deterministic), use_transmittance=int(transmittance),
                                    xy_raw_stride=stride, debug=0, reserved2=0, opacity_exponent=exponent, opacity_scale=scale,
                                    inv_w=inv_w, inv_h=inv_h, logits=logits.data_ptr(), xy_raw=xy_raw.data_ptr(),
                                    ray_xy=ray_xy.data_ptr(), near=near.data_ptr(), far=far.data_ptr(), index=index.data_ptr(), **more)

    @staticmethod
    def backward(ctx, g_depth, g_opacity, g_coords, _g_index):
        logits, xy_raw, ray_xy, near, far, index = ctx.saved_tensors
        dev = logits.device
        ptr = lambda t: None if t is None else t.data_ptr()
        f = lambda t: None if t is None else t.to(dtype=torch.float32).contiguous()
        g_depth, g_opacity, g_coords = f(g_depth), f(g_opacity), f(g_coords)
        d_logits = _depth_head_buffer(tuple(logits.shape), torch.float32, dev)
        d_xy = _depth_head_buffer(tuple(xy_raw.shape), torch.float32, dev) if ctx.needs_input_grad[1] else None
        dp = _FusedDepthHead._pass(ctx.dims, logits, xy_raw, ray_xy, near, far, index, dL_ddepth=ptr(g_depth),
                                   dL_dopacity=ptr(g_opacity), dL_dcoords=ptr(g_coords), dL_dlogits=d_logits.data_ptr(),
                                   dL_dxy_raw=ptr(d_xy))
        with torch.cuda.device(dev):
            rc = _lib.load().ggr_depth_head_backward(C.byref(dp), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"ggr_depth_head_backward failed (code {rc}): {_lib.last_error()}")
        return d_logits if ctx.needs_input_grad[0] else None, d_xy, None, None, None, None, None


def fused_depth_head(logits: Tensor, xy_raw: Tensor, ray_xy: Tensor, near: Tensor, far: Tensor, image_shape, num_surfaces: int,
                     samples_per_ray: int, deterministic: bool, *, use_transmittance: bool = False, opacity_exponent: float = 1.0,
                     opacity_scale: Optional[float] = None, u: Optional[Tensor] = None) -> DepthHead:
    """GGRt's ``DepthPredictorMonocular.forward`` after its projection, ``map_pdf_to_opacity`` / gaussians_per_pixel and the
    pixel-offset lines of ``EncoderEpipolar.forward`` as one HIP launch, and one more for the backward (the
    arithmetic: ``GgrDepthHeadPass`` in include/ggr_raster.h).  C = b·v cameras of R rays: ``logits`` [C,R,2·s·srf] is
    ``depth_predictor.projection``'s output in its own channel order ``(dpt srf c)``; ``xy_raw`` [C,R·srf,2] (or [C,R,srf,2]) the
    first two channels of the ``to_gaussians`` rows — a view whose rows have one common stride and a unit inner stride, such as
    ``rows[..., :2]``, is read in place, anything else is made contiguous; ``ray_xy`` [R,2] the normalised pixel centres;
    ``near`` / ``far`` [C]; ``image_shape`` (h, w) gives the pixel size.  ``deterministic``: the ``samples_per_ray`` buckets of
    largest pdf, ties to the lower bucket; otherwise one bucket per uniform number of ``u`` [C,R,srf,spp] (``None``: drawn here
    with ``torch.rand`` on the device — the kernel draws nothing).  ``opacity_exponent`` is the reference's ``2**x`` for the
    current ``global_step``; ``opacity_scale=None`` means ``1 / samples_per_ray``.  Returns ``DepthHead`` with G = R·srf·spp
    Gaussians per camera, sample axis innermost: what ``fused_gaussian_adapter(ext, intr, coordinates, depths, rows[..., 2:], …)``
    and the decoder's ``opacities`` (``.reshape(b, -1)``, a view) take.  Gradients reach ``logits`` and ``xy_raw``; the choice
    of ``index`` is not differentiated and ``near``, ``far``, ``ray_xy``, ``u`` get none."""
    dev = logits.device
    if dev.type != "cuda":
        raise RuntimeError("fused_depth_head runs on the GPU only (there is no CPU fallback)")
    srf, spp = int(num_surfaces), int(samples_per_ray)
    if logits.dim() != 3 or srf < 1 or logits.shape[-1] % (2 * srf) != 0 or logits.shape[-1] == 0:
        raise ValueError(f"logits {tuple(logits.shape)} is not [C, R, 2*s*{srf}]")
    n_cam, rays, width = logits.shape
    s = width // (2 * srf)
    if tuple(xy_raw.shape) not in ((n_cam, rays * srf, 2), (n_cam, rays, srf, 2)):
        raise ValueError(f"xy_raw {tuple(xy_raw.shape)} is neither [{n_cam}, {rays * srf}, 2] nor [{n_cam}, {rays}, {srf}, 2]")
    if tuple(ray_xy.shape) != (rays, 2) or near.numel() != n_cam or far.numel() != n_cam:
        raise ValueError("ray_xy must be [R, 2], near and far [C]")
    h, w = image_shape
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    logits = f(logits)
    xy_raw = xy_raw.to(device=dev, dtype=torch.float32).reshape(n_cam, rays * srf, 2)
    if not (xy_raw.stride(2) == 1 and xy_raw.stride(1) >= 2 and (n_cam < 2 or xy_raw.stride(0) == xy_raw.stride(1) * rays * srf)):
        xy_raw = xy_raw.contiguous()
    if not deterministic:
        if u is None:
            u = torch.rand((n_cam, rays, srf, spp), dtype=torch.float32, device=dev)
        if u.numel() != n_cam * rays * srf * spp:
            raise ValueError(f"u {tuple(u.shape)} is not [{n_cam}, {rays}, {srf}, {spp}]")
        u = f(u.detach())
    else:
        u = None
    scale = 1.0 / spp if opacity_scale is None else float(opacity_scale)
    dims = (n_cam, rays, s, srf, spp, bool(deterministic), bool(use_transmittance), float(opacity_exponent), scale, 1.0 / w, 1.0 / h)
    depth, opacity, coords, index = _FusedDepthHead.apply(logits, xy_raw, f(ray_xy.detach()), f(near.detach().reshape(-1)),
                                                          f(far.detach().reshape(-1)), u, dims)
    return DepthHead(depths=depth, opacities=opacity, coordinates=coords, index=index)


@dataclass
class EpipolarSamples:
    """What ``fused_epipolar_sampler`` returns: the fields of the reference's ``EpipolarSampling`` and ``depth``."""
    features: Tensor         # [b, v, v-1, r, s, c]   (differentiable with respect to the feature maps)
    valid: Tensor            # [b, v, v-1, r] bool
    xy_ray: Tensor           # [b, v, r, 2]
    xy_sample: Tensor        # [b, v, v-1, r, s, 2]
    xy_sample_near: Tensor   # [b, v, v-1, r, s, 2]
    xy_sample_far: Tensor    # [b, v, v-1, r, s, 2]
    origins: Tensor          # [b, v, r, 3]
    directions: Tensor       # [b, v, r, 3]
    depth: Tensor            # [b, v, v-1, r, s]: the relative disparity that the depth encoding takes


def _epipolar_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {_lib.last_error()}")


class _FusedEpipolarSampler(torch.autograd.Function):
    """ggr_epipolar_forward / ggr_epipolar_backward (csrc/epipolar.hip) behind autograd.  `images` [b,v,c,h,w] is read through
    its strides; the cameras arrive detached, float32 and contiguous."""

    @staticmethod
    def forward(ctx, images, c2w, w2c, K, Kinv, near, far, dims):
        dev = images.device
        b, v, c, h, w, s, window = dims
        r = h * w if window is None else (window[1] - window[0]) * (window[3] - window[2])
        pairs = (b, v, v - 1, r)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        out = dict(features=new(pairs + (s, c)), valid=new(pairs, torch.uint8), xy_ray=new((b, v, r, 2)), xy_sample=new(pairs + (s, 2)),
                   xy_sample_near=new(pairs + (s, 2)), xy_sample_far=new(pairs + (s, 2)), origins=new((b, v, r, 3)),
                   directions=new((b, v, r, 3)), depth=new(pairs + (s,)), segment=new(pairs + (4,)))
        lib = _lib.load()
        nbytes = max(int(lib.ggr_epipolar_scratch_bytes(b, v, c, h, w)), 0)
        scratch = new((nbytes // 4,))
        ep = _FusedEpipolarSampler._pass(dims, images=images.data_ptr(), image_strides=images.stride(), c2w=c2w.data_ptr(),
                                         w2c=w2c.data_ptr(), K=K.data_ptr(), Kinv=Kinv.data_ptr(), near=near.data_ptr(),
                                         far=far.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=nbytes,
                                         **{k: t.data_ptr() for k, t in out.items()})
        with torch.cuda.device(dev):
            _epipolar_check(lib.ggr_epipolar_forward(C.byref(ep), torch.cuda.current_stream(dev).cuda_stream), "ggr_epipolar_forward")
        ctx.dims = dims
        ctx.save_for_backward(out["valid"], out["segment"])
        rest = tuple(out[k] for k in ("valid", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions", "depth"))
        ctx.mark_non_differentiable(*rest)
        return (out["features"],) + rest

    @staticmethod
    def _pass(dims, **more):
        b, v, c, h, w, s, window = dims
        y0, y1, x0, x1 = window if window is not None else (0, 0, 0, 0)
        return _lib.epipolar_pass(reserved=0, batch=b, num_views=v, channels=c, height=h, width=w, num_samples=s,
                                  use_window=int(window is not None), window_y0=y0, window_y1=y1, window_x0=x0, window_x1=x1, debug=0, **more)

    @staticmethod
    def backward(ctx, g_features, *_others):
        valid, segment = ctx.saved_tensors
        b, v, c, h, w, s, window = ctx.dims
        dev = valid.device
        g_features = g_features.to(dtype=torch.float32).contiguous()
        d_images = torch.empty((b, v, c, h, w), dtype=torch.float32, device=dev)
        lib = _lib.load()
        nbytes = max(int(lib.ggr_epipolar_scratch_bytes(b, v, c, h, w)), 0)
        scratch = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        ep = _FusedEpipolarSampler._pass(ctx.dims, valid=valid.data_ptr(), segment=segment.data_ptr(), dL_dfeatures=g_features.data_ptr(),
                                         dL_dimages=d_images.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=nbytes)
        with torch.cuda.device(dev):
            _epipolar_check(lib.ggr_epipolar_backward(C.byref(ep), torch.cuda.current_stream(dev).cuda_stream), "ggr_epipolar_backward")
        return d_images, None, None, None, None, None, None, None


def fused_epipolar_sampler(images: Tensor, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, num_samples: int,
                           ray_window=None) -> EpipolarSamples:
    """GGRt's ``EpipolarSampler.forward`` and the depth lines of ``EpipolarTransformer.forward`` (``get_depth``, the clip to
    [near, far], ``depth_to_relative_disparity``) as HIP launches (the arithmetic: ``GgrEpipolarPass`` in
    include/ggr_raster.h).  ``images`` [b,v,c,h,w] are the (downscaled) feature maps, ``extrinsics`` [b,v,4,4] camera-to-world,
    ``intrinsics`` [b,v,3,3] normalised, ``near`` / ``far`` [b,v].  ``ray_window`` = (y0, y1, x0, x1) in ray-grid units casts only
    the rays of that sub-rectangle of every view (the reference's ``crop_size`` path: rows ``h//crop*clip_h`` to
    ``h//crop*(clip_h+1)``, columns alike); the feature maps stay whole.  Returns ``EpipolarSamples``: ``features`` is
    differentiable with respect to ``images`` (one scatter launch, float atomics: reproducible up to summation order);
    everything else is returned detached.  Camera gradients are not implemented: a camera tensor that requires grad raises.
    ``images`` may be any float32 view (it is read through its strides); another dtype is converted once."""
    dev = images.device
    if dev.type != "cuda":
        raise RuntimeError("fused_epipolar_sampler runs on the GPU only (there is no CPU fallback)")
    for name, t in (("extrinsics", extrinsics), ("intrinsics", intrinsics), ("near", near), ("far", far)):
        if t.requires_grad:
            raise RuntimeError(f"fused_epipolar_sampler: {name} requires grad, but camera gradients are not implemented here "
                               "(GGRt detaches its context poses; detach the cameras, near and far)")
    if images.dim() != 5:
        raise ValueError(f"images {tuple(images.shape)} is not [b, v, c, h, w]")
    b, v, c, h, w = images.shape
    if tuple(extrinsics.shape) != (b, v, 4, 4) or tuple(intrinsics.shape) != (b, v, 3, 3) or tuple(near.shape) != (b, v) or tuple(far.shape) != (b, v):
        raise ValueError(f"extrinsics must be [{b}, {v}, 4, 4], intrinsics [{b}, {v}, 3, 3], near and far [{b}, {v}]")
    window = None if ray_window is None else tuple(int(q) for q in ray_window)
    if window is not None and not (len(window) == 4 and 0 <= window[0] < window[1] <= h and 0 <= window[2] < window[3] <= w):
        raise ValueError(f"ray_window {window} is not (y0, y1, x0, x1) inside the {h} x {w} ray grid")
    if images.dtype != torch.float32:
        images = images.to(dtype=torch.float32)
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    c2w, K = f(extrinsics), f(intrinsics)
    w2c, Kinv = torch.linalg.inv(c2w).contiguous(), torch.linalg.inv(K).contiguous()
    dims = (b, v, c, h, w, int(num_samples), window)
    out = _FusedEpipolarSampler.apply(images, c2w, w2c, K, Kinv, f(near), f(far), dims)
    return EpipolarSamples(features=out[0], valid=out[1].bool(), xy_ray=out[2], xy_sample=out[3], xy_sample_near=out[4],
                           xy_sample_far=out[5], origins=out[6], directions=out[7], depth=out[8])


class _EpipolarAttentionCore(torch.autograd.Function):
    """ggr_epipolar_attention_forward / _backward (csrc/epipolar_attn.hip) behind autograd: qk [N,H,C], z [N,S,C], float32 and
    contiguous on arrival → ctx [N,H,C], attn [N,H,S].  attn is the only tensor saved beside the inputs."""

    @staticmethod
    def _call(name, dev, dims, **pointers):
        n, s, c, h = dims
        ap = _lib.epipolar_attn_pass(reserved=0, N=n, S=s, C=c, H=h, **pointers)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), name)(C.byref(ap), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")

    @staticmethod
    def forward(ctx, qk, z):
        dev = z.device
        (n, h, c), s = qk.shape, z.shape[1]
        out = torch.empty((n, h, c), dtype=torch.float32, device=dev)
        attn = torch.empty((n, h, s), dtype=torch.float32, device=dev)
        _EpipolarAttentionCore._call("ggr_epipolar_attention_forward", dev, (n, s, c, h), qk=qk.data_ptr(), z=z.data_ptr(),
                                     out_ctx=out.data_ptr(), out_attn=attn.data_ptr())
        ctx.save_for_backward(qk, z, attn)
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    def backward(ctx, g_out, _g_attn):
        qk, z, attn = ctx.saved_tensors
        dev = z.device
        (n, h, c), s = qk.shape, z.shape[1]
        g_out = g_out.to(dtype=torch.float32).contiguous()
        g_qk, g_z = torch.empty_like(qk), torch.empty_like(z)
        _EpipolarAttentionCore._call("ggr_epipolar_attention_backward", dev, (n, s, c, h), qk=qk.data_ptr(), z=z.data_ptr(),
                                     attn=attn.data_ptr(), dL_dctx=g_out.data_ptr(), dL_dqk=g_qk.data_ptr(), dL_dz=g_z.data_ptr())
        return g_qk, g_z


def epipolar_attention_core(qk: Tensor, z: Tensor):
    """The per-ray part of GGRt's epipolar cross-attention as one HIP launch, and one more for the backward (INTEGRATION.md §25;
    the arithmetic: ``GgrEpipolarAttnPass`` in include/ggr_raster.h).  ``qk`` [N,H,C] is the query with the key projection folded
    in, ``z`` [N,S,C] the ray's raw samples.  Returns ``(ctx, attn)``: ``ctx[n,h] = Σ_s attn[n,h,s]·z[n,s]`` [N,H,C],
    differentiable with respect to both inputs, and ``attn = softmax_s(qk·z)`` [N,H,S], detached (for visualisation).  Two runs
    give the same bits, forward and backward."""
    if qk.device.type != "cuda" or z.device.type != "cuda":
        raise RuntimeError("epipolar_attention_core runs on the GPU only (there is no CPU fallback)")
    if qk.dim() != 3 or z.dim() != 3 or qk.shape[0] != z.shape[0] or qk.shape[2] != z.shape[2]:
        raise ValueError(f"qk {tuple(qk.shape)} is not [N, H, C] for z {tuple(z.shape)} = [N, S, C]")
    f = lambda t: t.to(device=z.device, dtype=torch.float32).contiguous()
    return _EpipolarAttentionCore.apply(f(qk), f(z))


def fused_epipolar_attention(x: Tensor, z: Tensor, w_q: Tensor, w_kv: Tensor, w_out: Optional[Tensor], b_out: Optional[Tensor],
                             heads: int, return_weights: bool = False):
    """GGRt's ``Attention.forward(x, z)`` (``transformer/attention.py:57-74``) where ``EpipolarTransformer.forward`` calls it: ONE
    query token per ray against the ray's S samples, without the key and value tensors.  ``x`` [N,dim] or
    [N,1,dim] (after the caller's LayerNorm), ``z`` [N,S,kv_dim] (not normed), ``w_q`` = ``to_q.weight`` [H·D,dim], ``w_kv`` =
    ``to_kv.weight`` [2·H·D,kv_dim], ``w_out`` / ``b_out`` = ``to_out[0]``'s weight [dim,H·D] and bias, or ``None`` for the
    reference's ``project_out = False`` (heads = 1, D = dim).  ``to_q``, the fold ``qk = scale·Wk_hᵀq_h``, ``Wv_h·ctx_h`` and
    ``to_out`` are [N,·]-sized torch GEMMs; the logits, the softmax over the samples and the weighted sum are
    ``epipolar_attention_core``.  Autograd gives every gradient (x, z and the weights).  Returns the result in ``x``'s shape — with
    ``return_weights`` also the attention weights [N,H,S], detached.  Dropout is not modelled (GGRt's is 0.0)."""
    if x.dim() == 3 and x.shape[1] != 1:
        raise ValueError(f"fused_epipolar_attention takes ONE query token per ray: x {tuple(x.shape)} has {x.shape[1]} "
                         "(more than one query token per ray is not implemented)")
    if x.device.type != "cuda" or z.device.type != "cuda":
        raise RuntimeError("fused_epipolar_attention runs on the GPU only (there is no CPU fallback)")
    if x.dim() not in (2, 3) or z.dim() != 3 or z.shape[0] != x.shape[0]:
        raise ValueError(f"x {tuple(x.shape)} is not [N, dim] or [N, 1, dim] for z {tuple(z.shape)} = [N, S, kv_dim]")
    heads = int(heads)
    n, dim, kv_dim = x.shape[0], x.shape[-1], z.shape[2]
    inner = w_q.shape[0]
    if heads < 1 or inner % heads != 0 or tuple(w_q.shape) != (inner, dim) or tuple(w_kv.shape) != (2 * inner, kv_dim):
        raise ValueError(f"w_q {tuple(w_q.shape)} must be [H*D, {dim}] and w_kv {tuple(w_kv.shape)} [2*H*D, {kv_dim}] with H = {heads}")
    if w_out is None and inner != dim:
        raise ValueError(f"without w_out the result is the heads' output itself: H*D = {inner} must equal dim = {dim}")
    d = inner // heads
    f32 = lambda t: t.to(dtype=torch.float32)
    q = (f32(x).reshape(n, dim) @ f32(w_q).t()).reshape(n, heads, d)
    wk, wv = f32(w_kv)[:inner].reshape(heads, d, kv_dim), f32(w_kv)[inner:].reshape(heads, d, kv_dim)
    qk = torch.einsum("nhd,hdc->nhc", q, wk * (d ** -0.5))      # (the scale on the [H,D,C] weights: no [N,H,C] temporary)
    ctx, attn = epipolar_attention_core(qk, z)
    del qk, q
    out = torch.einsum("nhc,hdc->nhd", ctx, wv).reshape(n, inner)
    if w_out is not None:
        out = torch.nn.functional.linear(out, f32(w_out), None if b_out is None else f32(b_out))
    out = out.reshape(x.shape)
    return (out, attn) if return_weights else out


def _enc_attn_call(name, dev, dims, **pointers):
    n, s, c, h, o = dims
    ap = _lib.epipolar_attn_enc_pass(reserved=0, N=n, S=s, C=c, H=h, num_octaves=o, reserved2=0, **pointers)
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(C.byref(ap), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")


def _enc_attn_forward(qk, qe, features, depth):
    """ggr_epipolar_attention_encoded_forward on float32, contiguous tensors → ctx_f [N,H,C], ctx_e [N,H,E], attn [N,H,S]"""
    dev = features.device
    (n, h, c), s, e = qk.shape, features.shape[1], qe.shape[2]
    out_f = torch.empty((n, h, c), dtype=torch.float32, device=dev)
    out_e = torch.empty((n, h, e), dtype=torch.float32, device=dev)
    attn = torch.empty((n, h, s), dtype=torch.float32, device=dev)
    _enc_attn_call("ggr_epipolar_attention_encoded_forward", dev, (n, s, c, h, e // 2), qk=qk.data_ptr(), qe=qe.data_ptr(),
                   features=features.data_ptr(), depth=depth.data_ptr(), out_ctx_f=out_f.data_ptr(), out_ctx_e=out_e.data_ptr(),
                   out_attn=attn.data_ptr())
    return out_f, out_e, attn


def _enc_attn_backward(qk, qe, features, depth, attn, g_f, g_e, depth_grad):
    """ggr_epipolar_attention_encoded_backward → g_qk, g_qe, g_features, g_depth (None unless `depth_grad`)"""
    dev = features.device
    (n, h, c), s, e = qk.shape, features.shape[1], qe.shape[2]
    g_f, g_e = g_f.to(dtype=torch.float32).contiguous(), g_e.to(dtype=torch.float32).contiguous()
    g_qk, g_qe, g_feat = torch.empty_like(qk), torch.empty_like(qe), torch.empty_like(features)
    g_d = torch.empty_like(depth) if depth_grad else None
    _enc_attn_call("ggr_epipolar_attention_encoded_backward", dev, (n, s, c, h, e // 2), qk=qk.data_ptr(), qe=qe.data_ptr(),
                   features=features.data_ptr(), depth=depth.data_ptr(), attn=attn.data_ptr(), dL_dctx_f=g_f.data_ptr(),
                   dL_dctx_e=g_e.data_ptr(), dL_dqk=g_qk.data_ptr(), dL_dqe=g_qe.data_ptr(), dL_dfeatures=g_feat.data_ptr(),
                   dL_ddepth=None if g_d is None else g_d.data_ptr())
    return g_qk, g_qe, g_feat, g_d


class _EpipolarEncodedAttentionCore(torch.autograd.Function):
    """ggr_epipolar_attention_encoded_forward / _backward (csrc/epipolar_attn_enc.hip) behind autograd: qk [N,H,C], qe [N,H,E],
    features [N,S,C], depth [N,S], float32 and contiguous on arrival → ctx_f [N,H,C], ctx_e [N,H,E], attn [N,H,S].  attn is the
    only tensor saved beside the inputs; dL/ddepth is computed only when depth asks for it."""

    @staticmethod
    def forward(ctx, qk, qe, features, depth):
        out_f, out_e, attn = _enc_attn_forward(qk, qe, features, depth)
        ctx.save_for_backward(qk, qe, features, depth, attn)
        ctx.mark_non_differentiable(attn)
        return out_f, out_e, attn

    @staticmethod
    def backward(ctx, g_f, g_e, _g_attn):
        return _enc_attn_backward(*ctx.saved_tensors, g_f, g_e, ctx.needs_input_grad[3])


class _EpipolarEncodedAttentionFolded(torch.autograd.Function):
    """The same with ``qe = qk @ w_enc`` inside: qk [N,H,C], w_enc [C,E], features, depth → ctx_f, ctx_e, attn.  The fold's
    backward adds ``g_qe @ w_encᵀ`` into the kernel's dL/dqk IN PLACE: left to autograd, the fold keeps qk, a second [N,H,C]
    gradient and their sum alive beside dL/dfeatures, at the peak of the whole step.  qe [N,H,E] is computed again in the
    backward instead of being saved."""

    @staticmethod
    def forward(ctx, qk, w_enc, features, depth):
        out_f, out_e, attn = _enc_attn_forward(qk, qk @ w_enc, features, depth)
        ctx.save_for_backward(qk, w_enc, features, depth, attn)
        ctx.mark_non_differentiable(attn)
        return out_f, out_e, attn

    @staticmethod
    def backward(ctx, g_f, g_e, _g_attn):
        qk, w_enc, features, depth, attn = ctx.saved_tensors
        g_qk, g_qe, g_feat, g_d = _enc_attn_backward(qk, qk @ w_enc, features, depth, attn, g_f, g_e, ctx.needs_input_grad[3])
        c, e = w_enc.shape
        g_w = qk.reshape(-1, c).t() @ g_qe.reshape(-1, e)
        g_qk.view(-1, c).addmm_(g_qe.view(-1, e), w_enc.t())
        return g_qk, g_w, g_feat, g_d


def epipolar_encoded_attention_core(qk: Tensor, qe: Tensor, features: Tensor, depth: Tensor):
    """``epipolar_attention_core`` on ``z = features + linear(PE(depth))`` without z, as one HIP launch, and one more for the
    backward (the arithmetic and the encoding's exact contract: ``GgrEpipolarAttnEncPass`` in
    include/ggr_raster.h).  ``qk`` [N,H,C] is the query with the key projection folded in, ``qe`` [N,H,2·O] = ``qk @ w_enc`` that
    query against the encoding's ``nn.Linear``, ``features`` [N,S,C] and ``depth`` [N,S] the sampler's.  Returns
    ``(ctx_f, ctx_e, attn)``: ``ctx_f[n,h] = Σ_s attn[n,h,s]·features[n,s]`` [N,H,C] and ``ctx_e[n,h] = Σ_s attn[n,h,s]·PE(depth[n,s])``
    [N,H,2·O], differentiable with respect to all four inputs (``depth`` only if it requires a gradient), and ``attn`` [N,H,S],
    detached.  The number of octaves O is ``qe.shape[-1] // 2``, 1..16.  Two runs give the same bits, forward and backward."""
    if any(t.device.type != "cuda" for t in (qk, qe, features, depth)):
        raise RuntimeError("epipolar_encoded_attention_core runs on the GPU only (there is no CPU fallback)")
    if qk.dim() != 3 or features.dim() != 3 or qk.shape[0] != features.shape[0] or qk.shape[2] != features.shape[2]:
        raise ValueError(f"qk {tuple(qk.shape)} is not [N, H, C] for features {tuple(features.shape)} = [N, S, C]")
    if qe.dim() != 3 or tuple(qe.shape[:2]) != tuple(qk.shape[:2]):
        raise ValueError(f"qe {tuple(qe.shape)} is not [N, H, 2*num_octaves] for qk {tuple(qk.shape)} = [N, H, C]")
    if qe.shape[2] % 2 != 0:
        raise ValueError(f"qe {tuple(qe.shape)}: the last dimension is 2*num_octaves (a sine and a cosine per octave), not the odd {qe.shape[2]}")
    if tuple(depth.shape) != tuple(features.shape[:2]):
        raise ValueError(f"depth {tuple(depth.shape)} is not [N, S] for features {tuple(features.shape)} = [N, S, C]")
    f = lambda t: t.to(device=features.device, dtype=torch.float32).contiguous()
    return _EpipolarEncodedAttentionCore.apply(f(qk), f(qe), f(features), f(depth))


def fused_epipolar_encoded_attention(x: Tensor, features: Tensor, depth: Tensor, w_enc: Tensor, b_enc: Optional[Tensor], w_q: Tensor,
                                     w_kv: Tensor, w_out: Optional[Tensor], b_out: Optional[Tensor], heads: int,
                                     return_weights: bool = False):
    """``fused_epipolar_attention(x, features + linear(PE(depth[..., None]), w_enc, b_enc), w_q, w_kv, w_out, b_out, heads)`` in
    value and in every gradient, without that z: GGRt's ``EpipolarTransformer.forward`` lines 120-121 and 157-160 on the sampler's
    own outputs.  ``features`` [N,S,C] and ``depth`` [N,S] are ``EpipolarSamples.features`` / ``.depth``
    reshaped, ``w_enc`` [C,2·O] and ``b_enc`` [C] (or None) the weight and bias of ``depth_encoding[1]``, PE the reference's
    ``PositionalEncoding(O)`` on its float32 constants; the rest as ``fused_epipolar_attention``.  The ``nn.Linear`` of the
    encoding turns into ``qe = qk @ w_enc`` before and ``(Wv_h·w_enc)·ctx_e_h + Wv_h·b_enc`` after the kernels of
    ``epipolar_encoded_attention_core``: [N·H,·]-sized GEMMs instead of one over N·S tokens.  Autograd gives every gradient (x, features, depth if it requires one,
    w_enc, b_enc and the attention's weights)."""
    if x.dim() == 3 and x.shape[1] != 1:
        raise ValueError(f"fused_epipolar_encoded_attention takes ONE query token per ray: x {tuple(x.shape)} has {x.shape[1]} "
                         "(more than one query token per ray is not implemented)")
    if x.device.type != "cuda" or features.device.type != "cuda" or depth.device.type != "cuda":
        raise RuntimeError("fused_epipolar_encoded_attention runs on the GPU only (there is no CPU fallback)")
    if x.dim() not in (2, 3) or features.dim() != 3 or features.shape[0] != x.shape[0]:
        raise ValueError(f"x {tuple(x.shape)} is not [N, dim] or [N, 1, dim] for features {tuple(features.shape)} = [N, S, kv_dim]")
    if tuple(depth.shape) != tuple(features.shape[:2]):
        raise ValueError(f"depth {tuple(depth.shape)} is not [N, S] for features {tuple(features.shape)} = [N, S, kv_dim]")
    heads = int(heads)
    n, dim, kv_dim = x.shape[0], x.shape[-1], features.shape[2]
    inner = w_q.shape[0]
    if w_enc.dim() != 2 or w_enc.shape[0] != kv_dim or w_enc.shape[1] % 2 != 0 or (b_enc is not None and tuple(b_enc.shape) != (kv_dim,)):
        raise ValueError(f"w_enc {tuple(w_enc.shape)} must be [{kv_dim}, 2*num_octaves] and b_enc [{kv_dim}] or None")
    if heads < 1 or inner % heads != 0 or tuple(w_q.shape) != (inner, dim) or tuple(w_kv.shape) != (2 * inner, kv_dim):
        raise ValueError(f"w_q {tuple(w_q.shape)} must be [H*D, {dim}] and w_kv {tuple(w_kv.shape)} [2*H*D, {kv_dim}] with H = {heads}")
    if w_out is None and inner != dim:
        raise ValueError(f"without w_out the result is the heads' output itself: H*D = {inner} must equal dim = {dim}")
    d = inner // heads
    f32 = lambda t: t.to(dtype=torch.float32)
    q = (f32(x).reshape(n, dim) @ f32(w_q).t()).reshape(n, heads, d)
    wk, wv = f32(w_kv)[:inner].reshape(heads, d, kv_dim), f32(w_kv)[inner:].reshape(heads, d, kv_dim)
    qk = torch.einsum("nhd,hdc->nhc", q, wk * (d ** -0.5))
    cont = lambda t: f32(t).contiguous()
    # qe = qk @ w_enc [N,H,E], the encoding's Linear on the query's side, is folded inside (and its backward adds into dL/dqk in place)
    ctx_f, ctx_e, attn = _EpipolarEncodedAttentionFolded.apply(qk.contiguous(), cont(w_enc), cont(features), cont(depth))
    del qk, q
    out = torch.einsum("nhc,hdc->nhd", ctx_f, wv)
    out = out + torch.einsum("nhe,hde->nhd", ctx_e, wv @ f32(w_enc))     # Wv_h·w_enc [H,D,E]: no [N,H,C] temporary
    if b_enc is not None:
        out = out + wv @ f32(b_enc)                                # Wv_h·b_enc [H,D]
    out = out.reshape(n, inner)
    if w_out is not None:
        out = torch.nn.functional.linear(out, f32(w_out), None if b_out is None else f32(b_out))
    out = out.reshape(x.shape)
    return (out, attn) if return_weights else out


class ImageLoss(NamedTuple):
    """What ``fused_image_loss`` returns: both fields are differentiable; shape [] with ``size_average``, otherwise [B]."""
    mse: Tensor
    ssim: Tensor

    @property
    def psnr(self) -> Tensor:
        """The reference's ``mse2psnr``: −10·log10(mse + 1e-6), a torch expression on ``mse``."""
        return -10.0 * torch.log10(self.mse + 1e-6)


# tests only: True fills every buffer the image-loss launches must write whole with NaN before the launch
_IMAGE_LOSS_POISON = False


def _image_loss_buffer(shape, dev, dtype=torch.float32):
    if _IMAGE_LOSS_POISON:
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)
    return torch.empty(shape, dtype=dtype, device=dev)


class _FusedImageLoss(torch.autograd.Function):
    """ggr_image_loss_forward / ggr_image_loss_backward (csrc/image_loss.hip) behind autograd: pred, target [B,C,H,W] and mask
    [B,H,W] or None, float32 and contiguous on arrival → mse, ssim.  Only the inputs and the mse denominator are saved."""

    @staticmethod
    def _call(name, dev, dims, **pointers):
        b, c, h, w, window, size_average = dims
        lp = _lib.image_loss_pass(reserved=0, batch=b, channels=c, height=h, width=w, window_size=window, size_average=int(size_average),
                                  **pointers)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), name)(C.byref(lp), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")

    @staticmethod
    def forward(ctx, pred, target, mask, window_size, size_average):
        dev = pred.device
        b, c, h, w = pred.shape
        dims = (b, c, h, w, window_size, size_average)
        shape = () if size_average else (b,)
        mse, ssim, scale = (_image_loss_buffer(shape, dev) for _ in range(3))
        nbytes = int(_lib.load().ggr_image_loss_partials_bytes(b, c, h, w))
        if nbytes < 0:
            raise ValueError(f"fused_image_loss: pred {tuple(pred.shape)} is larger than the pass takes")
        partials = _image_loss_buffer((nbytes // 8,), dev, torch.float64)
        _FusedImageLoss._call("ggr_image_loss_forward", dev, dims, pred=pred.data_ptr(), target=target.data_ptr(),
                              mask=None if mask is None else mask.data_ptr(), out_mse=mse.data_ptr(), out_ssim=ssim.data_ptr(),
                              mse_scale=scale.data_ptr(), partials=partials.data_ptr(), partials_bytes=nbytes)
        ctx.dims = dims
        ctx.has_mask = mask is not None
        ctx.set_materialize_grads(False)     # (a field nobody used arrives as None and goes to the launch as NULL)
        ctx.save_for_backward(pred, target, scale, *(() if mask is None else (mask,)))
        return mse, ssim

    @staticmethod
    def backward(ctx, g_mse, g_ssim):
        if g_mse is None and g_ssim is None:
            return None, None, None, None, None
        pred, target, scale = ctx.saved_tensors[:3]
        mask = ctx.saved_tensors[3] if ctx.has_mask else None
        dev = pred.device
        ptr = lambda t: None if t is None else t.data_ptr()
        f = lambda t: None if t is None else t.to(dtype=torch.float32).contiguous()
        g_mse, g_ssim = f(g_mse), f(g_ssim)
        d_pred = _image_loss_buffer(tuple(pred.shape), dev) if ctx.needs_input_grad[0] else None
        d_target = _image_loss_buffer(tuple(pred.shape), dev) if ctx.needs_input_grad[1] else None
        if d_pred is not None or d_target is not None:
            _FusedImageLoss._call("ggr_image_loss_backward", dev, ctx.dims, pred=pred.data_ptr(), target=target.data_ptr(), mask=ptr(mask),
                                  mse_scale=scale.data_ptr(), dL_dmse=ptr(g_mse), dL_dssim=ptr(g_ssim), dL_dpred=ptr(d_pred),
                                  dL_dtarget=ptr(d_target))
        return d_pred, d_target, None, None, None


def fused_image_loss(pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, *, window_size: int = 11,
                     size_average: bool = True) -> ImageLoss:
    """GGRt's training loss ``img2mse(x, y, mask)`` (``utils_loc.py``) and its evaluation metric ``ssim(img1, img2, window_size,
    size_average)`` (``ggrt/loss/ssim_torch.py``) of a rendered image against its target as one HIP launch plus a small finishing
    one, and one launch per image for the backward (the arithmetic: ``GgrImageLossPass`` in
    include/ggr_raster.h).  ``pred`` / ``target`` [B,C,H,W] float32 on the GPU — or [C,H,W], the rasterizer's own output, taken as
    B = 1; ``mask`` [B,H,W] (or [H,W]) float weights of the MSE, which is then Σ d²·mask / (Σ mask·C + 1e-6); the mask does not
    enter SSIM and gets no gradient.  ``size_average=False`` gives one value per image, each MSE with its own mask slice.  Returns
    ``ImageLoss(mse, ssim)`` (and ``.psnr``): both differentiable with respect to ``pred`` and ``target``; a field that the loss does
    not use costs nothing in the backward (with ``mse`` alone the backward is one element-wise pass).  Non-contiguous inputs are
    made contiguous; two runs give the same bits."""
    for name, t in (("pred", pred), ("target", target), ("mask", mask)):
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"fused_image_loss: {name} is not a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"fused_image_loss: {name} is on {t.device}; the pass runs on the GPU only (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"fused_image_loss: {name} is {t.dtype}, not torch.float32")
    if pred.dim() not in (3, 4):
        raise ValueError(f"fused_image_loss: pred {tuple(pred.shape)} is neither [B, C, H, W] nor [C, H, W]")
    if tuple(target.shape) != tuple(pred.shape):
        raise ValueError(f"fused_image_loss: target {tuple(target.shape)} does not have the shape of pred {tuple(pred.shape)}")
    if target.device != pred.device or (mask is not None and mask.device != pred.device):
        raise RuntimeError("fused_image_loss: pred, target and mask are not on one device")
    window_size = int(window_size)
    if window_size < 1 or window_size > 11 or window_size % 2 == 0:
        raise ValueError(f"fused_image_loss: window_size {window_size} is not an odd number in 1..11")
    if pred.numel() == 0:
        raise ValueError(f"fused_image_loss: pred {tuple(pred.shape)} has no elements")
    batched = pred.dim() == 4
    if mask is not None:
        if mask.requires_grad:
            raise RuntimeError("fused_image_loss: mask requires grad, but there is no gradient with respect to the mask (detach it)")
        want = (pred.shape[0],) + tuple(pred.shape[2:]) if batched else tuple(pred.shape[1:])
        if tuple(mask.shape) != want:
            raise ValueError(f"fused_image_loss: mask {tuple(mask.shape)} is not {list(want)} for pred {tuple(pred.shape)}")
        mask = (mask if batched else mask[None]).contiguous()
    if not batched:
        pred, target = pred[None], target[None]
    mse, ssim = _FusedImageLoss.apply(pred.contiguous(), target.contiguous(), mask, window_size, bool(size_average))
    return ImageLoss(mse=mse, ssim=ssim)


def fused_ssim(img1: Tensor, img2: Tensor, window_size: int = 11, size_average: bool = True) -> Tensor:
    """The reference's ``ssim(img1, img2, window_size, size_average)`` (``ggrt/loss/ssim_torch.py``) with the same signature and
    meaning, through ``fused_image_loss``: differentiable with respect to both images."""
    return fused_image_loss(img1, img2, None, window_size=window_size, size_average=size_average).ssim


class PhotometricLoss(NamedTuple):
    """What ``fused_photometric_loss`` returns.  ``loss`` [1] is differentiable; ``photometric_loss`` and ``smoothness_loss`` [] are
    the reference's two metrics, detached; ``thresholds`` [n, C] the clip values; ``choice`` [n, H, W] uint8 the candidate that won
    each pixel's minimum (``choice % 2 == 1`` is Monodepth2's auto-mask), or None without ``return_choice``."""
    loss: Tensor
    photometric_loss: Tensor
    smoothness_loss: Tensor
    thresholds: Tensor
    choice: Optional[Tensor]


PHOTOMETRIC_MAX_CANDIDATES = 16     # kPhotoMaxCandidates of csrc/photometric_loss.h: V <= 8 with the auto-mask, V <= 16 without


class _FusedPhotometricLoss(torch.autograd.Function):
    """ggr_photometric_loss_forward / _backward (csrc/photometric_loss.hip) behind autograd: float32 contiguous tensors on arrival
    (inv_depths [n,H,W], poses [V,n,6]) → loss, metrics, thresholds, choice.  The candidate planes, the thresholds, the choice
    and 2n numbers of state are saved; every buffer comes from torch."""

    @staticmethod
    def _call(name, dev, dims, opts, **pointers):
        v, n, h, w, automask = dims
        lp = _lib.photometric_loss_pass(reserved=0, num_views=v, num_iters=n, height=h, width=w, automask=int(automask), reserved2=0,
                                        **opts, **pointers)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), name)(C.byref(lp), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")

    @staticmethod
    def forward(ctx, inv_depths, poses, image, ref_imgs, K, ref_Ks, automask, opts):
        dev = image.device
        n, h, w = inv_depths.shape
        v = ref_imgs.shape[0]
        dims = (v, n, h, w, automask)
        c = v * (2 if automask else 1)
        lib = _lib.load()
        planes_bytes, ws_bytes = int(lib.ggr_photometric_loss_planes_bytes(v, n, h, w, int(automask))), int(lib.ggr_photometric_loss_workspace_bytes(v, n, h, w, int(automask)))
        if planes_bytes < 0 or ws_bytes < 0:
            raise ValueError(f"fused_photometric_loss: {v} views x {n} iterations at {h} x {w} is more than the pass takes")
        planes = _image_loss_buffer((planes_bytes // 4,), dev)
        workspace = _image_loss_buffer((ws_bytes // 8,), dev, torch.float64)
        thresholds, state = _image_loss_buffer((n, c), dev), _image_loss_buffer((2 * n,), dev)
        choice = torch.full((n, h, w), 255, dtype=torch.uint8, device=dev) if _IMAGE_LOSS_POISON else torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        loss, photo, smooth = _image_loss_buffer((1,), dev), _image_loss_buffer((), dev), _image_loss_buffer((), dev)
        fixed = dict(image=image.data_ptr(), ref_imgs=ref_imgs.data_ptr(), inv_depths=inv_depths.data_ptr(), K=K.data_ptr(), ref_Ks=ref_Ks.data_ptr(),
                     poses=poses.data_ptr(), planes=planes.data_ptr(), planes_bytes=planes_bytes, out_thresholds=thresholds.data_ptr(),
                     state=state.data_ptr(), choice=choice.data_ptr())
        _FusedPhotometricLoss._call("ggr_photometric_loss_forward", dev, dims, opts, workspace=workspace.data_ptr(), workspace_bytes=ws_bytes,
                                    out_loss=loss.data_ptr(), out_photometric=photo.data_ptr(), out_smoothness=smooth.data_ptr(), **fixed)
        ctx.dims, ctx.opts, ctx.ws_bytes, ctx.planes_bytes = dims, opts, ws_bytes, planes_bytes
        ctx.save_for_backward(inv_depths, poses, image, ref_imgs, K, ref_Ks, planes, thresholds, state, choice)
        ctx.mark_non_differentiable(photo, smooth, thresholds, choice)
        ctx.set_materialize_grads(False)
        return loss, photo, smooth, thresholds, choice

    @staticmethod
    def backward(ctx, g_loss, *_):
        if g_loss is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 8
        inv_depths, poses, image, ref_imgs, K, ref_Ks, planes, thresholds, state, choice = ctx.saved_tensors
        dev = image.device
        g_loss = g_loss.to(dtype=torch.float32).contiguous()
        workspace = _image_loss_buffer((ctx.ws_bytes // 8,), dev, torch.float64)
        d_inv, d_poses = _image_loss_buffer(tuple(inv_depths.shape), dev), _image_loss_buffer(tuple(poses.shape), dev)
        _FusedPhotometricLoss._call("ggr_photometric_loss_backward", dev, ctx.dims, ctx.opts, image=image.data_ptr(), ref_imgs=ref_imgs.data_ptr(),
                                    inv_depths=inv_depths.data_ptr(), K=K.data_ptr(), ref_Ks=ref_Ks.data_ptr(), poses=poses.data_ptr(),
                                    planes=planes.data_ptr(), planes_bytes=ctx.planes_bytes, out_thresholds=thresholds.data_ptr(),
                                    state=state.data_ptr(), choice=choice.data_ptr(), workspace=workspace.data_ptr(), workspace_bytes=ctx.ws_bytes,
                                    dL_dloss=g_loss.data_ptr(), dL_dinv_depths=d_inv.data_ptr(), dL_dposes=d_poses.data_ptr())
        return (d_inv if ctx.needs_input_grad[0] else None, d_poses if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


def fused_photometric_loss(image: Tensor, ref_imgs: Tensor, inv_depths, K: Tensor, ref_Ks: Tensor, poses: Tensor, *,
                           ssim_loss_weight: float = 0.85, smooth_loss_weight: float = 0.01, C1: float = 1e-4, C2: float = 9e-4,
                           clip_loss: float = 0.5, automask_loss: bool = True, gamma: float = 0.85, return_choice: bool = False,
                           padding_mode: str = "zeros", photometric_reduce_op: str = "min") -> PhotometricLoss:
    """GGRt's ``MultiViewPhotometricDecayLoss.forward(image, ref_imgs, inv_depths, K, ref_Ks, poses)`` (``ggrt/loss/
    photometric_loss.py``) as four HIP launches forward and two backward, whatever the numbers of iterations and views
    (the arithmetic: ``GgrPhotometricLossPass`` in include/ggr_raster.h).  ``image`` [1,3,H,W] or [3,H,W];
    ``ref_imgs`` [V,3,H,W]; ``inv_depths`` a list of n tensors [1,1,H,W], as the reference receives it, or one [n,1,H,W] tensor;
    ``K`` [1,3,3]; ``ref_Ks`` [V,3,3]; ``poses`` [V,n,6], translation first, then the Euler angles of ``Pose.from_vec``; all float32 on
    the GPU.  Returns ``PhotometricLoss(loss [1], photometric_loss [], smoothness_loss [], thresholds [n,C], choice [n,H,W] uint8 |
    None)`` with C = 2V candidates per pixel (V without ``automask_loss``) in the reference's order: warped 0, unwarped 0, warped 1 …

    ``loss`` is differentiable with respect to ``inv_depths`` and ``poses`` ONLY: the images and the intrinsics are data and get no
    gradient (one that requires grad is refused).  The gradient reaches each pixel's winning candidate, and only where it was not
    clamped; the thresholds ``mean + clip_loss·std`` are constants of the backward, as the reference's ``float()`` makes them, and
    stay on the device: nothing synchronises with the host.  Ties of the minimum go to the LOWEST candidate index (with an identity
    pose the warped image equals the unwarped one and the warped candidate wins).  ``photometric_loss`` is what the reference's
    metric of that name holds — with the smoothness term on that is the whole loss, because the reference adds the term in place
    to the tensor the metric shares its memory with.  ``clip_loss=0`` switches the clamp off, ``smooth_loss_weight=0`` skips the
    smoothness term.  Two runs give the same bits.

    Refused with a ValueError (use the reference's torch module for these): a batch other than 1; inverse-depth maps that are not at
    the image's resolution; ``ssim_loss_weight <= 0`` (the reference then has 3 candidate planes per view); a ``padding_mode``
    other than 'zeros' or a reduce other than 'min'; H or W below 2; V·n = 0; more than 16 candidates per pixel (V above 8 with the
    auto-mask, above 16 without)."""
    torch_route = "use the reference's torch module (MultiViewPhotometricDecayLoss) for that form"
    if padding_mode != "zeros":
        raise ValueError(f"fused_photometric_loss: padding_mode {padding_mode!r} is not 'zeros'; {torch_route}")
    if photometric_reduce_op != "min":
        raise ValueError(f"fused_photometric_loss: photometric_reduce_op {photometric_reduce_op!r} is not 'min'; {torch_route}")
    if isinstance(inv_depths, (list, tuple)):
        if len(inv_depths) == 0:
            raise ValueError(f"fused_photometric_loss: no inverse-depth maps (V·n = 0); {torch_route}")
        for d in inv_depths:
            if not torch.is_tensor(d) or d.dim() != 4 or d.shape[0] != 1 or d.shape[1] != 1:
                raise ValueError(f"fused_photometric_loss: an inverse-depth map is not a [1, 1, H, W] tensor (a batch other than 1?); {torch_route}")
        if any(tuple(d.shape) != tuple(inv_depths[0].shape) for d in inv_depths):
            raise ValueError(f"fused_photometric_loss: the inverse-depth maps are not all at one resolution; {torch_route}")
        inv_depths = torch.cat(list(inv_depths), 0)
    tensors = (("image", image), ("ref_imgs", ref_imgs), ("inv_depths", inv_depths), ("K", K), ("ref_Ks", ref_Ks), ("poses", poses))
    for name, t in tensors:
        if not torch.is_tensor(t):
            raise ValueError(f"fused_photometric_loss: {name} is not a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"fused_photometric_loss: {name} is on {t.device}; the pass runs on the GPU only (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"fused_photometric_loss: {name} is {t.dtype}, not torch.float32")
        if t.device != image.device:
            raise RuntimeError("fused_photometric_loss: the inputs are not on one device")
    for name, t in (("image", image), ("ref_imgs", ref_imgs), ("K", K), ("ref_Ks", ref_Ks)):
        if t.requires_grad:
            raise RuntimeError(f"fused_photometric_loss: {name} requires grad, but the images and intrinsics are data here: there is no gradient "
                               "with respect to them (detach it)")
    if image.dim() == 4:
        if image.shape[0] != 1:
            raise ValueError(f"fused_photometric_loss: image {tuple(image.shape)} has a batch other than 1; {torch_route}")
        image = image[0]
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"fused_photometric_loss: image {tuple(image.shape)} is neither [1, 3, H, W] nor [3, H, W]")
    h, w = int(image.shape[1]), int(image.shape[2])
    if h < 2 or w < 2:
        raise ValueError(f"fused_photometric_loss: image {h} x {w} is below 2 x 2 (reflection padding needs two pixels); {torch_route}")
    if ref_imgs.dim() != 4 or tuple(ref_imgs.shape[1:]) != (3, h, w):
        raise ValueError(f"fused_photometric_loss: ref_imgs {tuple(ref_imgs.shape)} is not [V, 3, {h}, {w}] (a batch other than 1?); {torch_route}")
    v = int(ref_imgs.shape[0])
    if inv_depths.dim() != 4 or inv_depths.shape[1] != 1:
        raise ValueError(f"fused_photometric_loss: inv_depths {tuple(inv_depths.shape)} is not [n, 1, H, W] (a batch other than 1?); {torch_route}")
    n = int(inv_depths.shape[0])
    if v * n == 0:
        raise ValueError(f"fused_photometric_loss: {v} views x {n} iterations is nothing (V·n = 0); {torch_route}")
    if tuple(inv_depths.shape[2:]) != (h, w):
        raise ValueError(f"fused_photometric_loss: inv_depths {tuple(inv_depths.shape[2:])} is not at the image's resolution {h} x {w}; {torch_route}")
    if tuple(K.shape) not in ((1, 3, 3), (3, 3)):
        raise ValueError(f"fused_photometric_loss: K {tuple(K.shape)} is not [1, 3, 3] (a batch other than 1?); {torch_route}")
    if tuple(ref_Ks.shape) != (v, 3, 3):
        raise ValueError(f"fused_photometric_loss: ref_Ks {tuple(ref_Ks.shape)} is not [{v}, 3, 3]")
    if tuple(poses.shape) != (v, n, 6):
        raise ValueError(f"fused_photometric_loss: poses {tuple(poses.shape)} is not [{v}, {n}, 6]")
    if not float(ssim_loss_weight) > 0.0:
        raise ValueError(f"fused_photometric_loss: ssim_loss_weight {ssim_loss_weight} is not above 0 (the reference then keeps three L1 planes per "
                         f"view); {torch_route}")
    if float(ssim_loss_weight) > 1.0:
        raise ValueError(f"fused_photometric_loss: ssim_loss_weight {ssim_loss_weight} is above 1")
    for name, x in (("smooth_loss_weight", smooth_loss_weight), ("C1", C1), ("C2", C2), ("clip_loss", clip_loss), ("gamma", gamma)):
        if not (float(x) >= 0.0 and float(x) < float("inf")):
            raise ValueError(f"fused_photometric_loss: {name} {x} is negative or not finite")
    c = v * (2 if automask_loss else 1)
    if c > PHOTOMETRIC_MAX_CANDIDATES:
        raise ValueError(f"fused_photometric_loss: {v} views make {c} candidates per pixel, more than the {PHOTOMETRIC_MAX_CANDIDATES} the pass is "
                         f"compiled for; {torch_route}")
    if n > 1024 or h > 16384 or w > 16384:
        raise ValueError(f"fused_photometric_loss: {n} iterations at {h} x {w} is more than the pass takes (1024, 16384 x 16384); {torch_route}")
    opts = dict(ssim_loss_weight=float(ssim_loss_weight), smooth_loss_weight=float(smooth_loss_weight), C1=float(C1), C2=float(C2),
                clip_loss=float(clip_loss), gamma=float(gamma))
    loss, photo, smooth, thresholds, choice = _FusedPhotometricLoss.apply(
        inv_depths.reshape(n, h, w).contiguous(), poses.contiguous(), image.contiguous(), ref_imgs.contiguous(), K.reshape(3, 3).contiguous(),
        ref_Ks.contiguous(), bool(automask_loss), opts)
    return PhotometricLoss(loss=loss, photometric_loss=photo, smoothness_loss=smooth, thresholds=thresholds, choice=choice if return_choice else None)


WARP_COST_MAX_VIEWS = 16     # kWarpMaxViews of csrc/warp_cost.h


class _FusedWarpCost(torch.autograd.Function):
    """ggr_warp_cost_forward / _backward (csrc/warp_cost.hip) behind autograd: float32 contiguous tensors on arrival (fmap [C,h,w],
    fmaps_ref [V,C,h,w], inv_depth [h,w], poses [V,6], K [3,3], ref_Ks [V,3,3]) → cost [V,C,h,w] or [1,C,h,w], cells [V,h,w,3] or
    None.  Only the inputs are saved: the backward recomputes the coordinates.  Every buffer comes from torch."""

    @staticmethod
    def _call(name, dev, dims, opts, **pointers):
        v, c, h, w = dims
        wp = _lib.warp_cost_pass(reserved=0, num_views=v, channels=c, height=h, width=w, reserved2=0, **opts, **pointers)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), name)(C.byref(wp), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")

    @staticmethod
    def forward(ctx, fmap, fmaps_ref, inv_depth, poses, K, ref_Ks, want_cells, opts):
        dev = fmap.device
        v, c, h, w = fmaps_ref.shape
        dims = (v, c, h, w)
        cost = _image_loss_buffer((1 if opts["reduce_mean"] else v, c, h, w), dev)
        cells = None
        if want_cells:
            cells = torch.full((v, h, w, 3), -(1 << 31), dtype=torch.int32, device=dev) if _IMAGE_LOSS_POISON else torch.empty((v, h, w, 3), dtype=torch.int32, device=dev)
        _FusedWarpCost._call("ggr_warp_cost_forward", dev, dims, opts, fmap=fmap.data_ptr(), fmaps_ref=fmaps_ref.data_ptr(), inv_depth=inv_depth.data_ptr(),
                             K=K.data_ptr(), ref_Ks=ref_Ks.data_ptr(), poses=poses.data_ptr(), out_cost=cost.data_ptr(),
                             out_cells=cells.data_ptr() if want_cells else None)
        ctx.dims, ctx.opts = dims, opts
        ctx.save_for_backward(fmap, fmaps_ref, inv_depth, poses, K, ref_Ks)
        ctx.set_materialize_grads(False)
        if want_cells:
            ctx.mark_non_differentiable(cells)
        return cost, cells

    @staticmethod
    def backward(ctx, g_cost, _g_cells=None):
        need = ctx.needs_input_grad[:4]
        if g_cost is None or not any(need):
            return (None,) * 8
        fmap, fmaps_ref, inv_depth, poses, K, ref_Ks = ctx.saved_tensors
        dev = fmap.device
        v, c, h, w = ctx.dims
        g_cost = g_cost.to(dtype=torch.float32).contiguous()
        outs = [_image_loss_buffer(tuple(t.shape), dev) if n else None for t, n in zip((fmap, fmaps_ref, inv_depth, poses), need)]
        if need[1]:         # the scatter adds into its output: a fill on the same stream, ahead of the launch
            outs[1] = torch.full(tuple(fmaps_ref.shape), 0.0, dtype=torch.float32, device=dev)
        ws_bytes = int(_lib.load().ggr_warp_cost_workspace_bytes(v, h, w)) if need[3] else 0
        workspace = _image_loss_buffer((ws_bytes // 8,), dev, torch.float64) if need[3] else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        _FusedWarpCost._call("ggr_warp_cost_backward", dev, ctx.dims, ctx.opts, fmap=fmap.data_ptr(), fmaps_ref=fmaps_ref.data_ptr(),
                             inv_depth=inv_depth.data_ptr(), K=K.data_ptr(), ref_Ks=ref_Ks.data_ptr(), poses=poses.data_ptr(),
                             workspace=ptr(workspace), workspace_bytes=ws_bytes, dL_dcost=g_cost.data_ptr(), dL_dfmap=ptr(outs[0]),
                             dL_dfmaps_ref=ptr(outs[1]), dL_dinv_depth=ptr(outs[2]), dL_dposes=ptr(outs[3]))
        return (*outs, None, None, None, None)


def fused_warp_cost(fmap: Tensor, fmaps_ref, inv_depth: Tensor, K: Tensor, ref_Ks: Tensor, poses, *, scale_factor: float = 1.0 / 8,
                    reduce: str = "mean", disp_range=None, return_cells: bool = False):
    """The feature-metric cost map of GGRt's ``DepthPoseNet`` (``ggrt/depth_pose_network.py``) for all V views in one HIP launch forward
    and two backward (the arithmetic: ``GgrWarpCostPass`` in include/ggr_raster.h).  ``reduce="mean"`` is
    ``depth_cost_calc(inv_depth, fmap, fmaps_ref, poses, K, ref_Ks, scale_factor)`` → [1,C,h,w]; ``reduce="none"`` is
    ``get_cost_each(poses[v], fmap, fmaps_ref[v], inv2depth(inv_depth), K, ref_Ks[v], scale_factor)`` for every v → [V,C,h,w].

    ``fmap`` [1,C,h,w] or [C,h,w]; ``fmaps_ref`` [V,C,h,w] or a list of V tensors [1,C,h,w] (the reference's tuple from
    ``torch.split``); ``inv_depth`` [1,1,h,w] at the maps' resolution; ``K`` [1,3,3] or [3,3] and ``ref_Ks`` [V,3,3], the
    FULL-resolution intrinsics, scaled inside by ``scale_factor`` as ``Camera.scaled`` does; ``poses`` [V,6] or a list of V tensors
    [1,6], translation first, then the Euler angles of ``Pose.from_vec``; all float32 on one GPU.  ``disp_range=(min_depth,
    max_depth)`` folds ``disp_to_depth``: ``inv_depth`` is then the raw sigmoid disparity.  ``return_cells=True`` returns ``(cost,
    cells)`` with ``cells`` [V,h,w,3] int32: the bilinear cell (floor u, floor v; (-2, -2) where no tap is reached) and the flag of a
    clamped ``P.z``, as the kernel decided them.

    Gradients reach ``fmap``, ``fmaps_ref``, ``inv_depth`` and ``poses``; one that does not require grad costs nothing.  The
    intrinsics are data (one that requires grad is refused).  ``dL/dfmaps_ref`` is scattered with float atomics; every other output
    is bit-reproducible.  No allocation inside, no host sync, graph-capturable.

    Refused with a ValueError (use the reference's torch route, ``DepthPoseNet.get_cost_each``, for these): a dtype other than
    float32; a CPU tensor; spatial sizes that differ between ``fmap``, ``fmaps_ref`` and ``inv_depth``; h or w below 2; V = 0 or above
    16; a batch other than 1; ``scale_factor <= 0``; a ``reduce`` other than "mean" or "none"; a ``disp_range`` that is not
    ``0 < min < max``."""
    torch_route = "use the reference's torch route (DepthPoseNet.get_cost_each / depth_cost_calc) for that form"
    if reduce not in ("mean", "none"):
        raise ValueError(f"fused_warp_cost: reduce {reduce!r} is neither 'mean' nor 'none'; {torch_route}")
    if not (isinstance(scale_factor, (int, float)) and float(scale_factor) > 0.0 and float(scale_factor) < float("inf")):
        raise ValueError(f"fused_warp_cost: scale_factor {scale_factor!r} is not a positive finite number; {torch_route}")
    if disp_range is not None:
        try:
            lo, hi = (float(x) for x in disp_range)
        except (TypeError, ValueError):
            raise ValueError(f"fused_warp_cost: disp_range {disp_range!r} is not a (min_depth, max_depth) pair; {torch_route}") from None
        if not (0.0 < lo < hi < float("inf")):
            raise ValueError(f"fused_warp_cost: disp_range {disp_range!r} is not 0 < min < max; {torch_route}")
    for name, seq, tail in (("fmaps_ref", fmaps_ref, 4), ("poses", poses, 2)):
        if isinstance(seq, (list, tuple)):
            if len(seq) == 0:
                raise ValueError(f"fused_warp_cost: {name} is empty (V = 0); {torch_route}")
            for t in seq:
                if not torch.is_tensor(t) or t.dim() != tail or t.shape[0] != 1:
                    raise ValueError(f"fused_warp_cost: an entry of {name} is not a tensor with a leading 1 (a batch other than 1?); {torch_route}")
            if any(tuple(t.shape) != tuple(seq[0].shape) or t.dtype != seq[0].dtype or t.device != seq[0].device for t in seq):
                raise ValueError(f"fused_warp_cost: the entries of {name} differ in shape (spatial sizes), dtype or device; {torch_route}")
    if isinstance(fmaps_ref, (list, tuple)):
        fmaps_ref = torch.cat(list(fmaps_ref), 0)
    if isinstance(poses, (list, tuple)):
        poses = torch.cat(list(poses), 0)
    tensors = (("fmap", fmap), ("fmaps_ref", fmaps_ref), ("inv_depth", inv_depth), ("K", K), ("ref_Ks", ref_Ks), ("poses", poses))
    for name, t in tensors:
        if not torch.is_tensor(t):
            raise ValueError(f"fused_warp_cost: {name} is not a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"fused_warp_cost: {name} is {t.dtype}, not torch.float32; {torch_route}")
    for name, t in tensors:
        if t.device.type != "cuda":
            raise ValueError(f"fused_warp_cost: {name} is on {t.device}; the pass runs on the GPU only (there is no CPU fallback); {torch_route}")
        if t.device != fmap.device:
            raise ValueError(f"fused_warp_cost: {name} is on {t.device}, fmap on {fmap.device}: the inputs are not on one device")
    for name, t in (("K", K), ("ref_Ks", ref_Ks)):
        if t.requires_grad:
            raise RuntimeError(f"fused_warp_cost: {name} requires grad, but the intrinsics are data here: there is no gradient with respect to "
                               "them (detach it)")
    if fmap.dim() == 4:
        if fmap.shape[0] != 1:
            raise ValueError(f"fused_warp_cost: fmap {tuple(fmap.shape)} has a batch other than 1; {torch_route}")
        fmap = fmap[0]
    if fmap.dim() != 3:
        raise ValueError(f"fused_warp_cost: fmap {tuple(fmap.shape)} is neither [1, C, h, w] nor [C, h, w]")
    c, h, w = (int(x) for x in fmap.shape)
    if c < 1:
        raise ValueError(f"fused_warp_cost: fmap {tuple(fmap.shape)} has no channels")
    if h < 2 or w < 2:
        raise ValueError(f"fused_warp_cost: fmap {h} x {w} is below 2 x 2 (align_corners divides by h - 1 and w - 1); {torch_route}")
    if fmaps_ref.dim() != 4:
        raise ValueError(f"fused_warp_cost: fmaps_ref {tuple(fmaps_ref.shape)} is not [V, C, h, w] (a batch other than 1?); {torch_route}")
    v = int(fmaps_ref.shape[0])
    if v == 0:
        raise ValueError(f"fused_warp_cost: fmaps_ref {tuple(fmaps_ref.shape)} holds no view (V = 0); {torch_route}")
    if v > WARP_COST_MAX_VIEWS:
        raise ValueError(f"fused_warp_cost: fmaps_ref holds {v} views, more than the {WARP_COST_MAX_VIEWS} the pass is compiled for; {torch_route}")
    if tuple(fmaps_ref.shape[1:]) != (c, h, w):
        raise ValueError(f"fused_warp_cost: fmaps_ref {tuple(fmaps_ref.shape)} does not have fmap's channels and spatial sizes [{c}, {h}, {w}]; {torch_route}")
    if inv_depth.dim() != 4 or inv_depth.shape[0] != 1 or inv_depth.shape[1] != 1:
        raise ValueError(f"fused_warp_cost: inv_depth {tuple(inv_depth.shape)} is not [1, 1, h, w] (a batch other than 1?); {torch_route}")
    if tuple(inv_depth.shape[2:]) != (h, w):
        raise ValueError(f"fused_warp_cost: inv_depth {tuple(inv_depth.shape[2:])} does not have fmap's spatial sizes {h} x {w}; {torch_route}")
    if h > 16384 or w > 16384 or c > 65536:
        raise ValueError(f"fused_warp_cost: fmap [{c}, {h}, {w}] is more than the pass takes (65536 channels, 16384 x 16384); {torch_route}")
    if tuple(K.shape) not in ((1, 3, 3), (3, 3)):
        raise ValueError(f"fused_warp_cost: K {tuple(K.shape)} is not [1, 3, 3] (a batch other than 1?); {torch_route}")
    if tuple(ref_Ks.shape) != (v, 3, 3):
        raise ValueError(f"fused_warp_cost: ref_Ks {tuple(ref_Ks.shape)} is not [{v}, 3, 3]")
    if tuple(poses.shape) != (v, 6):
        raise ValueError(f"fused_warp_cost: poses {tuple(poses.shape)} is not [{v}, 6]")
    opts = dict(reduce_mean=int(reduce == "mean"), fold_disp=int(disp_range is not None), scale_factor=float(scale_factor),
                min_depth=float(disp_range[0]) if disp_range is not None else 0.0, max_depth=float(disp_range[1]) if disp_range is not None else 0.0)
    cost, cells = _FusedWarpCost.apply(fmap.contiguous(), fmaps_ref.contiguous(), inv_depth.reshape(h, w).contiguous(), poses.contiguous(),
                                       K.reshape(3, 3).contiguous(), ref_Ks.contiguous(), bool(return_cells), opts)
    return (cost, cells) if return_cells else cost


UPSAMPLE_DEPTH_MAX_RATIO = 8     # kUpsampleMaxRatio of csrc/upsample_depth.h


class _FusedUpsampleDepth(torch.autograd.Function):
    """ggr_upsample_depth_forward / _backward (csrc/upsample_depth.hip) behind autograd: float32 contiguous tensors on arrival (depth
    [N,1,h,w], mask [N,9 r r,h,w]) → out [N,1,Ho,Wo].  Only the inputs are saved: the backward recomputes the softmax.  Every
    buffer, the workspace included, comes from torch."""

    @staticmethod
    def _call(name, dev, dims, opts, **pointers):
        n, h, w, r, ho, wo = dims
        ws_bytes = int(_lib.load().ggr_upsample_depth_workspace_bytes(n, h, w, r))
        if ws_bytes < 0:
            raise ValueError(f"fused_upsample_depth: {n} maps of {h} x {w} cells at ratio {r} are more than the pass indexes (2^31 - 1 elements "
                             "in the mask, sides of 65536); use the reference's torch route (DepthPoseNet.upsample_depth) for that form")
        workspace = _image_loss_buffer((ws_bytes // 4,), dev)
        up = _lib.upsample_depth_pass(reserved=0, batch=n, height=h, width=w, ratio=r, out_height=ho, out_width=wo, reserved2=0,
                                      workspace=workspace.data_ptr(), workspace_bytes=ws_bytes, **opts, **pointers)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), name)(C.byref(up), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")

    @staticmethod
    def forward(ctx, depth, mask, dims, opts):
        dev = depth.device
        n, h, w, r, ho, wo = dims
        out = _image_loss_buffer((n, 1, ho, wo), dev)
        _FusedUpsampleDepth._call("ggr_upsample_depth_forward", dev, dims, opts, depth=depth.data_ptr(), mask=mask.data_ptr(), out=out.data_ptr())
        ctx.dims, ctx.opts = dims, opts
        ctx.save_for_backward(depth, mask)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        need = ctx.needs_input_grad[:2]
        if g_out is None or not any(need):
            return (None,) * 4
        depth, mask = ctx.saved_tensors
        dev = depth.device
        g_out = g_out.to(dtype=torch.float32).contiguous()
        g_depth = _image_loss_buffer(tuple(depth.shape), dev) if need[0] else None
        g_mask = _image_loss_buffer(tuple(mask.shape), dev) if need[1] else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        _FusedUpsampleDepth._call("ggr_upsample_depth_backward", dev, ctx.dims, ctx.opts, depth=depth.data_ptr(), mask=mask.data_ptr(),
                                  dL_dout=g_out.data_ptr(), dL_dmask=ptr(g_mask), dL_ddepth=ptr(g_depth))
        return g_depth, g_mask, None, None


def fused_upsample_depth(depth, mask, *, ratio: int = 8, image_size=None, disp_range=None) -> Tensor:
    """The convex depth upsampling of GGRt's ``DepthPoseNet`` (``ggrt/depth_pose_network.py``) in two HIP launches forward and two
    backward (the arithmetic: ``GgrUpsampleDepthPass`` in include/ggr_raster.h):
    ``upsample_depth(depth, mask, ratio, image_size)`` and, with ``disp_range=(min_depth, max_depth)``,
    ``disp_to_depth(..., min_depth, max_depth)[0]`` of it → [N,1,Ho,Wo].

    ``depth`` [N,1,h,w] or [N,h,w], ``mask`` [N,9·ratio²,h,w], or a list or tuple of such maps and as many masks, stacked along N:
    the predictions of one ``DepthPoseNet.forward`` in one call.  ``image_size=None`` is (ratio·h, ratio·w), where the resize is the
    identity.  All float32 on one GPU; inputs that are not contiguous (a ``channels_last`` mask) are made so.

    Gradients reach ``depth`` and ``mask``; one that does not require grad costs nothing.  Both are gathers with a fixed order of
    summation: two runs give the same bits.  No host sync, graph-capturable; the workspace (the size of ``up``) is a torch buffer.

    Refused with a ValueError (use the reference's torch route, ``DepthPoseNet.upsample_depth``, for these): a dtype other than
    float32; a CPU tensor; a mask whose channel count is not 9·ratio² or whose batch or spatial sizes differ from ``depth``'s; a
    ``ratio`` outside 1..8; an ``image_size`` that is not two positive ints; a ``disp_range`` that is not ``0 < min < max``; an empty
    map or list."""
    torch_route = "use the reference's torch route (DepthPoseNet.upsample_depth) for that form"
    if not (isinstance(ratio, int) and not isinstance(ratio, bool) and 1 <= ratio <= UPSAMPLE_DEPTH_MAX_RATIO):
        raise ValueError(f"fused_upsample_depth: ratio {ratio!r} is not an int in 1..{UPSAMPLE_DEPTH_MAX_RATIO}; {torch_route}")
    if disp_range is not None:
        try:
            lo, hi = (float(x) for x in disp_range)
        except (TypeError, ValueError):
            raise ValueError(f"fused_upsample_depth: disp_range {disp_range!r} is not a (min_depth, max_depth) pair; {torch_route}") from None
        if not (0.0 < lo < hi < float("inf")):
            raise ValueError(f"fused_upsample_depth: disp_range {disp_range!r} is not 0 < min < max; {torch_route}")
    if isinstance(depth, (list, tuple)) != isinstance(mask, (list, tuple)):
        raise ValueError(f"fused_upsample_depth: depth and mask must both be tensors or both be lists; {torch_route}")
    if isinstance(depth, (list, tuple)):
        if len(depth) == 0 or len(depth) != len(mask):
            raise ValueError(f"fused_upsample_depth: depth holds {len(depth)} maps and mask {len(mask)}: the lists are empty or differ in length; {torch_route}")
        depths, masks = list(depth), list(mask)
    else:
        depths, masks = [depth], [mask]
    for name, seq in (("depth", depths), ("mask", masks)):
        for t in seq:
            if not torch.is_tensor(t):
                raise ValueError(f"fused_upsample_depth: {name} is not a tensor (or a list of tensors)")
            if t.dtype != torch.float32:
                raise ValueError(f"fused_upsample_depth: {name} is {t.dtype}, not torch.float32; {torch_route}")
    for name, seq in (("depth", depths), ("mask", masks)):
        for t in seq:
            if t.device.type != "cuda":
                raise ValueError(f"fused_upsample_depth: {name} is on {t.device}; the pass runs on the GPU only (there is no CPU fallback); {torch_route}")
            if t.device != depths[0].device:
                raise ValueError(f"fused_upsample_depth: {name} is on {t.device}, depth on {depths[0].device}: the inputs are not on one device")
    for k, d in enumerate(depths):
        if d.dim() == 3:
            depths[k] = d = d.unsqueeze(1)
        if d.dim() != 4 or d.shape[1] != 1:
            raise ValueError(f"fused_upsample_depth: depth {tuple(d.shape)} is neither [N, 1, h, w] nor [N, h, w]; {torch_route}")
        m = masks[k]
        if m.dim() != 4:
            raise ValueError(f"fused_upsample_depth: mask {tuple(m.shape)} is not [N, 9 * ratio^2, h, w]; {torch_route}")
        if m.shape[1] != 9 * ratio * ratio:
            raise ValueError(f"fused_upsample_depth: mask has {m.shape[1]} channels, not 9 * ratio^2 = {9 * ratio * ratio} at ratio {ratio}; {torch_route}")
        if m.shape[0] != d.shape[0] or tuple(m.shape[2:]) != tuple(d.shape[2:]):
            raise ValueError(f"fused_upsample_depth: mask {tuple(m.shape)} does not have depth's batch and spatial sizes {tuple(d.shape)}; {torch_route}")
        if tuple(d.shape[2:]) != tuple(depths[0].shape[2:]):
            raise ValueError(f"fused_upsample_depth: the maps of the depth list differ in spatial sizes ({tuple(d.shape[2:])} and {tuple(depths[0].shape[2:])}); {torch_route}")
    depth = depths[0] if len(depths) == 1 else torch.cat(depths, 0)
    mask = masks[0] if len(masks) == 1 else torch.cat(masks, 0)
    n, _, h, w = (int(x) for x in depth.shape)
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"fused_upsample_depth: depth {tuple(depth.shape)} is empty; {torch_route}")
    if image_size is None:
        ho, wo = ratio * h, ratio * w
    else:
        try:
            ho, wo = image_size
        except (TypeError, ValueError):
            raise ValueError(f"fused_upsample_depth: image_size {image_size!r} is not a (height, width) pair; {torch_route}") from None
        if not all(isinstance(x, int) and not isinstance(x, bool) and x >= 1 for x in (ho, wo)):
            raise ValueError(f"fused_upsample_depth: image_size {image_size!r} is not two positive ints; {torch_route}")
    opts = dict(fold_disp=int(disp_range is not None), min_depth=float(disp_range[0]) if disp_range is not None else 0.0,
                max_depth=float(disp_range[1]) if disp_range is not None else 0.0)
    return _FusedUpsampleDepth.apply(depth.contiguous(), mask.contiguous(), (n, h, w, ratio, int(ho), int(wo)), opts)


_GRU_TORCH_ROUTE = "use the reference's torch route (SepConvGRU.forward / ConvGRU.forward of ggrt/optimizer.py) for that form"
_GRU_DA_Z_MARK = "_ggr_gru_da_z"     # set on what _GruBlend.backward returns for z: the z half of a [N,2Ch,H,W] dL/da_zr buffer


def _gru_call(name, dev, dims, **pointers):
    n, ch, hh, ww = dims
    gp = _lib.gru_pass(reserved=0, batch=n, channels=ch, height=hh, width=ww, **pointers)
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(C.byref(gp), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")


def _gru_ptr(t):
    return t.data_ptr() if t is not None else None


class _GruGate(torch.autograd.Function):
    """ggr_gru_gate_forward / _backward (csrc/gru_gates.hip) behind autograd: a_zr_h, a_zr_x (or None) [N,2Ch,H,W] and h [N,Ch,H,W],
    float32 contiguous on arrival → (z, rh).  Saves r and h.  The gradient that arrives for z is not dL/dz: it is what
    `_GruBlend.backward` returns for its z, the z half of a dL/da_zr buffer whose r half this backward fills in place, so that the one
    array serves as the gradient of both pre-activations.  Any other gradient for z (z used by something else than `gru_blend`, or by
    two of them) is refused."""

    @staticmethod
    def forward(ctx, a_zr_h, a_zr_x, h):
        dev, dims = h.device, tuple(int(v) for v in h.shape)
        z, r, rh = (_image_loss_buffer(dims, dev) for _ in range(3))
        _gru_call("ggr_gru_gate_forward", dev, dims, a_zr_h=a_zr_h.data_ptr(), a_zr_x=_gru_ptr(a_zr_x), h=h.data_ptr(), z=z.data_ptr(),
                  r=r.data_ptr(), rh=rh.data_ptr())
        ctx.dims = dims
        ctx.save_for_backward(r, h)
        ctx.set_materialize_grads(False)
        return z, rh

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_rh):
        need_a, need_h = ctx.needs_input_grad[0] or ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if (g_z is None and g_rh is None) or not (need_a or need_h):
            return None, None, None
        r, h = ctx.saved_tensors
        dev, (n, ch, hh, ww) = h.device, ctx.dims
        g_a_zr = None
        if need_a:
            if g_z is None:             # the gate used alone: nothing reaches a_zr's z half
                g_a_zr = _image_loss_buffer((n, 2 * ch, hh, ww), dev)
                g_a_zr[:, :ch].zero_()
            else:
                g_a_zr = g_z._base if getattr(g_z, _GRU_DA_Z_MARK, False) else None
                if (g_a_zr is None or tuple(g_a_zr.shape) != (n, 2 * ch, hh, ww) or not g_a_zr.is_contiguous() or g_a_zr.dtype != torch.float32
                        or g_z.data_ptr() != g_a_zr.data_ptr()):
                    raise RuntimeError("gru_gate: z is differentiable through one gru_blend only (its gradient slot carries dL/da_z, which "
                                       "gru_blend's backward forms); another use of z received or added a gradient")
        g_h = None
        if g_rh is None:                # rh unused: r has no gradient, and h none through it
            if g_a_zr is not None:
                g_a_zr[:, ch:].zero_()
        else:
            g_rh = g_rh.to(dtype=torch.float32).contiguous()
            g_h = _image_loss_buffer((n, ch, hh, ww), dev) if need_h else None
            _gru_call("ggr_gru_gate_backward", dev, ctx.dims, dL_drh=g_rh.data_ptr(), r=r.data_ptr(), h=h.data_ptr(), dL_da_zr=_gru_ptr(g_a_zr),
                      dL_dh=_gru_ptr(g_h))
        return (g_a_zr if ctx.needs_input_grad[0] else None, g_a_zr if ctx.needs_input_grad[1] else None, g_h)


class _GruBlend(torch.autograd.Function):
    """ggr_gru_blend_forward / _backward behind autograd: a_q_h, a_q_x (or None), z, h [N,Ch,H,W] → h'.  Saves z, q and h.  What its
    backward returns for z is dL/da_z (`_GruGate`)."""

    @staticmethod
    def forward(ctx, a_q_h, a_q_x, z, h):
        dev, dims = h.device, tuple(int(v) for v in h.shape)
        q, out = _image_loss_buffer(dims, dev), _image_loss_buffer(dims, dev)
        _gru_call("ggr_gru_blend_forward", dev, dims, a_q_h=a_q_h.data_ptr(), a_q_x=_gru_ptr(a_q_x), z=z.data_ptr(), h=h.data_ptr(),
                  q=q.data_ptr(), out_h=out.data_ptr())
        ctx.dims = dims
        ctx.save_for_backward(z, q, h)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        need = ctx.needs_input_grad
        need_q = need[0] or need[1]
        if g is None or not (need_q or need[2] or need[3]):
            return None, None, None, None
        z, q, h = ctx.saved_tensors
        dev, (n, ch, hh, ww) = h.device, ctx.dims
        g = g.to(dtype=torch.float32).contiguous()
        g_a_q = _image_loss_buffer((n, ch, hh, ww), dev) if need_q else None
        g_a_zr = _image_loss_buffer((n, 2 * ch, hh, ww), dev) if need[2] else None
        g_h = _image_loss_buffer((n, ch, hh, ww), dev) if need[3] else None
        _gru_call("ggr_gru_blend_backward", dev, ctx.dims, dL_dout_h=g.data_ptr(), z=z.data_ptr(), q=q.data_ptr(), h=h.data_ptr(),
                  dL_da_q=_gru_ptr(g_a_q), dL_da_zr=_gru_ptr(g_a_zr), dL_dh_part=_gru_ptr(g_h))
        g_z = None
        if g_a_zr is not None:
            g_z = g_a_zr[:, :ch]
            setattr(g_z, _GRU_DA_Z_MARK, True)
        return (g_a_q if need[0] else None, g_a_q if need[1] else None, g_z, g_h)


def _gru_maps(fn, first, maps):
    """The shared refusals of the GRU entry points: `maps` is [(name, tensor or None, channels or None)]; every tensor must be
    float32, on one GPU, 4-D, and have `first`'s batch and spatial sizes (and the given channel count)."""
    ref_name, ref = first
    for name, t, _ in maps:
        if t is not None and not torch.is_tensor(t):
            raise ValueError(f"{fn}: {name} is not a tensor; {_GRU_TORCH_ROUTE}")
    for name, t, _ in maps:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} is {t.dtype}, not torch.float32; {_GRU_TORCH_ROUTE}")
    for name, t, _ in maps:
        if t is not None and t.device.type != "cuda":
            raise ValueError(f"{fn}: {name} is on {t.device}; the kernels run on the GPU only (there is no CPU fallback); {_GRU_TORCH_ROUTE}")
    for name, t, _ in maps:
        if t is not None and t.device != ref.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, {ref_name} on {ref.device}: the inputs are not on one device; {_GRU_TORCH_ROUTE}")
    if ref.dim() != 4:
        raise ValueError(f"{fn}: {ref_name} {tuple(ref.shape)} is not [N, C, H, W]; {_GRU_TORCH_ROUTE}")
    if ref.shape[0] < 1 or ref.numel() == 0:
        raise ValueError(f"{fn}: {ref_name} {tuple(ref.shape)} is empty; {_GRU_TORCH_ROUTE}")
    for name, t, c in maps:
        if t is None:
            continue
        if t.dim() != 4 or t.shape[0] != ref.shape[0] or tuple(t.shape[2:]) != tuple(ref.shape[2:]):
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} does not have {ref_name}'s batch and spatial sizes {tuple(ref.shape)}; {_GRU_TORCH_ROUTE}")
        if c is not None and t.shape[1] != c:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} has {t.shape[1]} channels, not {c}; {_GRU_TORCH_ROUTE}")
    if 2 * ref.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: {ref_name} {tuple(ref.shape)} is more than the kernels index (N * 2 * Ch * H * W must stay below 2^31); {_GRU_TORCH_ROUTE}")


def gru_gate(a_zr_h: Tensor, a_zr_x: Optional[Tensor], h: Tensor):
    """The GRU's gates in one HIP launch each way (``GgrGruPass`` in include/ggr_raster.h): ``z = σ(a_zr_h[:, :Ch] + a_zr_x[:, :Ch])``,
    ``r = σ(a_zr_h[:, Ch:] + a_zr_x[:, Ch:])``, ``rh = r·h`` → ``(z, rh)``.  ``a_zr_h`` and ``a_zr_x`` are the [N,2Ch,H,W]
    pre-activations of the h-side and the x-side convolutions (``a_zr_x=None``: one convolution of a ``cat``), ``h`` [N,Ch,H,W].

    ``z`` is made for :func:`gru_blend`: it is differentiable through exactly one ``gru_blend``, whose backward hands the gate
    dL/da_z in z's gradient slot; a gradient from any other use of ``z`` raises a RuntimeError in the backward (``z.detach()`` is
    free to use).  ``rh`` is an ordinary differentiable tensor."""
    _gru_maps("gru_gate", ("h", h), [("h", h, None), ("a_zr_h", a_zr_h, 2 * h.shape[1] if torch.is_tensor(h) and h.dim() == 4 else None),
                                     ("a_zr_x", a_zr_x, 2 * h.shape[1] if torch.is_tensor(h) and h.dim() == 4 else None)])
    return _GruGate.apply(a_zr_h.contiguous(), a_zr_x.contiguous() if a_zr_x is not None else None, h.contiguous())


def gru_blend(a_q_h: Tensor, a_q_x: Optional[Tensor], z: Tensor, h: Tensor) -> Tensor:
    """The GRU's candidate and blend in one HIP launch each way: ``q = tanh(a_q_h + a_q_x)``, ``h' = (1 − z)·h + z·q`` → ``h'`` (a new
    tensor).  All [N,Ch,H,W]; ``a_q_x=None``: no second addend.  ``z`` is :func:`gru_gate`'s (or any tensor that needs no gradient)."""
    c = h.shape[1] if torch.is_tensor(h) and h.dim() == 4 else None
    _gru_maps("gru_blend", ("h", h), [("h", h, None), ("a_q_h", a_q_h, c), ("a_q_x", a_q_x, c), ("z", z, c)])
    return _GruBlend.apply(a_q_h.contiguous(), a_q_x.contiguous() if a_q_x is not None else None, z.contiguous(), h.contiguous())


def fused_gru_half(h: Tensor, x: Tensor, w_zr_h: Tensor, w_zr_x: Tensor, b_zr: Optional[Tensor], w_q_h: Tensor, w_q_x: Tensor,
                   b_q: Optional[Tensor], padding) -> Tensor:
    """One half-step of GGRt's ``SepConvGRU`` (or the whole step of ``ConvGRU``, ``ggrt/optimizer.py``) with its three convolutions
    over ``cat[h, x]`` split by input and its pointwise chain in two HIP launches each way::

        a_zr_h = conv(h, w_zr_h)      a_zr_x = conv(x, w_zr_x, b_zr)      a_q_x = conv(x, w_q_x, b_q)
        z, rh  = gru_gate(a_zr_h, a_zr_x, h)
        a_q_h  = conv(rh, w_q_h)
        h'     = gru_blend(a_q_h, a_q_x, z, h)

    ``h`` [N,Ch,H,W], ``x`` [N,Cx,H,W]; ``w_zr_h`` [2Ch,Ch,kh,kw] and ``w_zr_x`` [2Ch,Cx,kh,kw] hold the z rows, then the r rows;
    ``w_q_h`` [Ch,Ch,kh,kw], ``w_q_x`` [Ch,Cx,kh,kw]; ``b_zr`` [2Ch] and ``b_q`` [Ch] (or None); ``padding`` = ((kh−1)/2, (kw−1)/2).
    The same function of the same parameters as the reference's half-step up to float32 summation order.  The convolutions are
    torch's; no ``cat`` and no [N,Ch+Cx,H,W] buffer is made.  Gradients reach every tensor argument that requires one.

    Refused with a ValueError that names the argument: a dtype other than float32, a CPU tensor, inputs on different devices, ``h``
    and ``x`` that differ in batch or spatial size, weights or biases whose shapes do not fit Ch / Cx / the padding, an empty batch."""
    ph, pw = _gru_half_check("fused_gru_half", h, x, w_zr_h, w_zr_x, b_zr, w_q_h, w_q_x, b_q, padding)
    h, x = h.contiguous(), x.contiguous()
    conv = torch.nn.functional.conv2d
    a_zr_h = conv(h, w_zr_h, None, padding=(ph, pw))
    a_zr_x = conv(x, w_zr_x, b_zr, padding=(ph, pw))
    a_q_x = conv(x, w_q_x, b_q, padding=(ph, pw))
    z, rh = _GruGate.apply(a_zr_h.contiguous(), a_zr_x.contiguous(), h)
    a_q_h = conv(rh, w_q_h, None, padding=(ph, pw))
    return _GruBlend.apply(a_q_h.contiguous(), a_q_x.contiguous(), z, h)


def _gru_half_check(fn, h, x, w_zr_h, w_zr_x, b_zr, w_q_h, w_q_x, b_q, padding):
    """The refusals that `fused_gru_half` and `fused_gru_half_inference` share → the padding as two ints."""
    tensors = [("h", h), ("x", x), ("w_zr_h", w_zr_h), ("w_zr_x", w_zr_x), ("b_zr", b_zr), ("w_q_h", w_q_h), ("w_q_x", w_q_x), ("b_q", b_q)]
    for name, t in tensors:
        if not (torch.is_tensor(t) or (t is None and name.startswith("b_"))):
            raise ValueError(f"{fn}: {name} is not a tensor; {_GRU_TORCH_ROUTE}")
    tensors = [(name, t) for name, t in tensors if t is not None]
    for name, t in tensors:
        if t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} is {t.dtype}, not torch.float32; {_GRU_TORCH_ROUTE}")
    for name, t in tensors:
        if t.device.type != "cuda":
            raise ValueError(f"{fn}: {name} is on {t.device}; the kernels run on the GPU only (there is no CPU fallback); {_GRU_TORCH_ROUTE}")
    for name, t in tensors:
        if t.device != h.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, h on {h.device}: the inputs are not on one device; {_GRU_TORCH_ROUTE}")
    if h.dim() != 4 or x.dim() != 4:
        raise ValueError(f"{fn}: h {tuple(h.shape)} and x {tuple(x.shape)} are not [N, Ch, H, W] and [N, Cx, H, W]; {_GRU_TORCH_ROUTE}")
    if h.shape[0] != x.shape[0] or tuple(h.shape[2:]) != tuple(x.shape[2:]):
        raise ValueError(f"{fn}: x {tuple(x.shape)} does not have h's batch and spatial sizes {tuple(h.shape)}; {_GRU_TORCH_ROUTE}")
    if h.numel() == 0 or x.numel() == 0:
        raise ValueError(f"{fn}: h {tuple(h.shape)} or x {tuple(x.shape)} is empty; {_GRU_TORCH_ROUTE}")
    try:
        ph, pw = (int(v) for v in padding)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: padding {padding!r} is not a (rows, columns) pair; {_GRU_TORCH_ROUTE}") from None
    ch, cx, kh, kw = int(h.shape[1]), int(x.shape[1]), 2 * ph + 1, 2 * pw + 1
    if ph < 0 or pw < 0:
        raise ValueError(f"{fn}: padding {padding!r} is negative; {_GRU_TORCH_ROUTE}")
    for name, t, want in (("w_zr_h", w_zr_h, (2 * ch, ch, kh, kw)), ("w_zr_x", w_zr_x, (2 * ch, cx, kh, kw)), ("b_zr", b_zr, (2 * ch,)),
                          ("w_q_h", w_q_h, (ch, ch, kh, kw)), ("w_q_x", w_q_x, (ch, cx, kh, kw)), ("b_q", b_q, (ch,))):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not {want} (Ch = {ch}, Cx = {cx}, padding {(ph, pw)}); {_GRU_TORCH_ROUTE}")
    if 2 * h.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: h {tuple(h.shape)} is more than the kernels index (N * 2 * Ch * H * W must stay below 2^31); {_GRU_TORCH_ROUTE}")
    return ph, pw


_GRU_TRAINING_ROUTE = "use fused_gru_half (torch's convolutions, which autograd differentiates) for that call"


def _gru_conv_refusals(fn, named, kh, kw):
    """What the forward-only convolution kernels (csrc/gru_conv.hip) refuse beyond the shapes: a gradient, kernel sides they do not have."""
    if torch.is_grad_enabled():
        for name, t in named:
            if t is not None and t.requires_grad:
                raise ValueError(f"{fn}: {name} requires grad and grad mode is on: this route is forward only; {_GRU_TRAINING_ROUTE}")
    if kh > 5 or kw > 5 or kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"{fn}: the padding gives a {kh} x {kw} kernel; the kernels take odd sides up to 5; {_GRU_TRAINING_ROUTE}")


def _gru_conv_call(dev, dims, kernel, epilogue, out_channels=0, **pointers):
    n, ch, cx, hh, ww = dims
    cp = _lib.gru_conv_pass(reserved=0, batch=n, channels=ch, in_channels=cx, height=hh, width=ww, kernel_h=kernel[0], kernel_w=kernel[1],
                            epilogue=epilogue, out_channels=out_channels, workspace=None, workspace_bytes=0, **pointers)
    lib = _lib.load()
    need = int(lib.ggr_gru_conv_workspace_bytes(C.byref(cp)))
    workspace = None
    if need:            # (0 today: the kernels pass nothing through memory)
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        cp.workspace, cp.workspace_bytes = workspace.data_ptr(), need
    with torch.cuda.device(dev):
        rc = lib.ggr_gru_conv_forward(C.byref(cp), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"ggr_gru_conv_forward failed (code {rc}): {_lib.last_error()}")


def fused_gru_half_inference(h: Tensor, x: Tensor, w_zr_h: Tensor, w_zr_x: Tensor, b_zr: Optional[Tensor], w_q_h: Tensor, w_q_x: Tensor,
                             b_q: Optional[Tensor], padding) -> Tensor:
    """`fused_gru_half` for a call that needs no gradient, with the convolutions in HIP as well: two launches of
    an implicit GEMM on the exact float32 MFMA (``GgrGruConvPass`` in include/ggr_raster.h) — GATE convolves ``h`` and ``x`` with the
    z/r weights and writes ``z`` and ``r·h``, BLEND convolves ``r·h`` and ``x`` with the q weights and writes ``h'``.  The
    pre-activations are never stored, the weights are read in place, nothing is cached and there is no autograd graph.  The same
    arguments and the same function as `fused_gru_half` up to float32 summation order.

    Refused as `fused_gru_half` refuses, and also, with a ValueError that names `fused_gru_half` as the route to take: a tensor
    argument that requires grad while grad mode is on, and a padding that makes a kernel side even or above 5."""
    fn = "fused_gru_half_inference"
    ph, pw = _gru_half_check(fn, h, x, w_zr_h, w_zr_x, b_zr, w_q_h, w_q_x, b_q, padding)
    named = (("h", h), ("x", x), ("w_zr_h", w_zr_h), ("w_zr_x", w_zr_x), ("b_zr", b_zr), ("w_q_h", w_q_h), ("w_q_x", w_q_x), ("b_q", b_q))
    kernel = (2 * ph + 1, 2 * pw + 1)
    _gru_conv_refusals(fn, named, *kernel)
    with torch.no_grad():
        h, x, w_zr_h, w_zr_x, w_q_h, w_q_x = (t.detach().contiguous() for t in (h, x, w_zr_h, w_zr_x, w_q_h, w_q_x))
        b_zr, b_q = (t.detach().contiguous() if t is not None else None for t in (b_zr, b_q))
        dev, shape = h.device, tuple(int(v) for v in h.shape)
        dims = (shape[0], shape[1], int(x.shape[1]), shape[2], shape[3])
        z, rh, out = (_image_loss_buffer(shape, dev) for _ in range(3))
        _gru_conv_call(dev, dims, kernel, _lib.GRU_CONV_GATE, a=h.data_ptr(), x=x.data_ptr(), w_h=w_zr_h.data_ptr(), w_x=w_zr_x.data_ptr(),
                       bias=_gru_ptr(b_zr), h=h.data_ptr(), z=z.data_ptr(), rh=rh.data_ptr())
        _gru_conv_call(dev, dims, kernel, _lib.GRU_CONV_BLEND, a=rh.data_ptr(), x=x.data_ptr(), w_h=w_q_h.data_ptr(), w_x=w_q_x.data_ptr(),
                       bias=_gru_ptr(b_q), h=h.data_ptr(), z=z.data_ptr(), out_h=out.data_ptr())
    return out


def gru_conv(a: Tensor, x: Tensor, w_h: Tensor, w_x: Tensor, bias: Optional[Tensor], padding) -> Tensor:
    """The split-input convolution of the GRU kernels alone (the RAW epilogue of ``GgrGruConvPass``), forward only::

        acc = conv2d(a, w_h, None, padding=padding) + conv2d(x, w_x, bias, padding=padding)

    in one HIP launch, without a ``cat`` — for a host that arranges its own tail.  ``a`` [N,Ca,H,W], ``x`` [N,Cx,H,W], ``w_h``
    [Cout,Ca,kh,kw], ``w_x`` [Cout,Cx,kh,kw], ``bias`` [Cout] or None, ``padding`` = ((kh−1)/2, (kw−1)/2) with odd sides up to 5
    → [N,Cout,H,W].  Exact float32 arithmetic in a fixed order: two calls give the same bits.  Refused with a ValueError that names
    the argument: what `fused_gru_half_inference` refuses, for these arguments."""
    fn = "gru_conv"
    tensors = [("a", a), ("x", x), ("w_h", w_h), ("w_x", w_x), ("bias", bias)]
    for name, t in tensors:
        if not (torch.is_tensor(t) or (t is None and name == "bias")):
            raise ValueError(f"{fn}: {name} is not a tensor; {_GRU_TRAINING_ROUTE}")
    tensors = [(name, t) for name, t in tensors if t is not None]
    for name, t in tensors:
        if t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} is {t.dtype}, not torch.float32; {_GRU_TRAINING_ROUTE}")
    for name, t in tensors:
        if t.device.type != "cuda":
            raise ValueError(f"{fn}: {name} is on {t.device}; the kernels run on the GPU only (there is no CPU fallback); {_GRU_TRAINING_ROUTE}")
    for name, t in tensors:
        if t.device != a.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, a on {a.device}: the inputs are not on one device; {_GRU_TRAINING_ROUTE}")
    if a.dim() != 4 or x.dim() != 4:
        raise ValueError(f"{fn}: a {tuple(a.shape)} and x {tuple(x.shape)} are not [N, Ca, H, W] and [N, Cx, H, W]; {_GRU_TRAINING_ROUTE}")
    if a.shape[0] != x.shape[0] or tuple(a.shape[2:]) != tuple(x.shape[2:]):
        raise ValueError(f"{fn}: x {tuple(x.shape)} does not have a's batch and spatial sizes {tuple(a.shape)}; {_GRU_TRAINING_ROUTE}")
    if a.numel() == 0 or x.numel() == 0:
        raise ValueError(f"{fn}: a {tuple(a.shape)} or x {tuple(x.shape)} is empty; {_GRU_TRAINING_ROUTE}")
    try:
        ph, pw = (int(v) for v in padding)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: padding {padding!r} is not a (rows, columns) pair; {_GRU_TRAINING_ROUTE}") from None
    if ph < 0 or pw < 0:
        raise ValueError(f"{fn}: padding {padding!r} is negative; {_GRU_TRAINING_ROUTE}")
    ca, cx, kh, kw = int(a.shape[1]), int(x.shape[1]), 2 * ph + 1, 2 * pw + 1
    if w_h.dim() != 4 or w_h.shape[0] < 1 or tuple(w_h.shape[1:]) != (ca, kh, kw):
        raise ValueError(f"{fn}: w_h {tuple(w_h.shape)} is not [Cout, {ca}, {kh}, {kw}] (Ca = {ca}, padding {(ph, pw)}); {_GRU_TRAINING_ROUTE}")
    cout = int(w_h.shape[0])
    for name, t, want in (("w_x", w_x, (cout, cx, kh, kw)), ("bias", bias, (cout,))):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not {want} (Cout = {cout}, Cx = {cx}, padding {(ph, pw)}); {_GRU_TRAINING_ROUTE}")
    n, hh, ww = int(a.shape[0]), int(a.shape[2]), int(a.shape[3])
    if n * hh * ww * max(2 * ca, cx, cout) >= 2 ** 31:
        raise ValueError(f"{fn}: a {tuple(a.shape)} with {cx} and {cout} channels beside it is more than the kernels index (every array must stay "
                         f"below 2^31 elements, a's twice over); {_GRU_TRAINING_ROUTE}")
    _gru_conv_refusals(fn, tensors, kh, kw)
    with torch.no_grad():
        a, x, w_h, w_x = (t.detach().contiguous() for t in (a, x, w_h, w_x))
        bias = bias.detach().contiguous() if bias is not None else None
        out = _image_loss_buffer((n, cout, hh, ww), a.device)
        _gru_conv_call(a.device, (n, ca, cx, hh, ww), (kh, kw), _lib.GRU_CONV_RAW, out_channels=cout, a=a.data_ptr(), x=x.data_ptr(),
                       w_h=w_h.data_ptr(), w_x=w_x.data_ptr(), bias=_gru_ptr(bias), raw=out.data_ptr())
    return out


class _FusedGRU(nn.Module):
    """The split parameters of a reference GRU and its forward through `fused_gru_half`.  HALVES lists (suffix of the reference's
    module names, kernel shape, padding) in the order the reference applies them."""
    HALVES: tuple = ()

    def __init__(self, hidden_dim: int = 128, input_dim: int = 192 + 128, *, hip_convs: bool = False):
        super().__init__()
        if not (isinstance(hidden_dim, int) and isinstance(input_dim, int) and hidden_dim >= 1 and input_dim >= 1):
            raise ValueError(f"{type(self).__name__}: hidden_dim {hidden_dim!r} and input_dim {input_dim!r} are not positive ints")
        self.hidden_dim, self.input_dim = hidden_dim, input_dim
        self.hip_convs = bool(hip_convs)
        ch, cx = hidden_dim, input_dim
        init = {}
        for s, (kh, kw), pad in self.HALVES:
            for name, shape in (("w_zr_h", (2 * ch, ch, kh, kw)), ("w_zr_x", (2 * ch, cx, kh, kw)), ("b_zr", (2 * ch,)), ("w_q_h", (ch, ch, kh, kw)),
                                ("w_q_x", (ch, cx, kh, kw)), ("b_q", (ch,))):
                setattr(self, name + s, nn.Parameter(torch.empty(shape)))
            for gate in "zrq":          # the reference's own initialisation: nn.Conv2d's, of the unsplit layer
                conv = nn.Conv2d(ch + cx, ch, (kh, kw), padding=pad)
                init[f"conv{gate}{s}.weight"], init[f"conv{gate}{s}.bias"] = conv.weight.detach(), conv.bias.detach()
        self.load_reference_state_dict(init)

    def _reference_keys(self):
        return [f"conv{gate}{s}.{what}" for s, _, _ in self.HALVES for gate in "zrq" for what in ("weight", "bias")]

    @torch.no_grad()
    def load_reference_state_dict(self, sd) -> None:
        """Takes the parameters of the reference module (its ``state_dict()``: ``convz1.weight`` … ``convq2.bias`` for ``SepConvGRU``,
        ``convz.weight`` … ``convq.bias`` for ``ConvGRU``), split by input channel and merged by gate.  Values are copied to the bit."""
        keys, ch, cx = self._reference_keys(), self.hidden_dim, self.input_dim
        if sorted(sd.keys()) != sorted(keys):
            raise ValueError(f"{type(self).__name__}.load_reference_state_dict: expected the keys {keys}, got {sorted(sd.keys())}")
        for s, (kh, kw), _ in self.HALVES:
            for gate in "zrq":
                w, b = sd[f"conv{gate}{s}.weight"], sd[f"conv{gate}{s}.bias"]
                if tuple(w.shape) != (ch, ch + cx, kh, kw) or tuple(b.shape) != (ch,):
                    raise ValueError(f"{type(self).__name__}.load_reference_state_dict: conv{gate}{s} has weight {tuple(w.shape)} and bias "
                                     f"{tuple(b.shape)}, not {(ch, ch + cx, kh, kw)} and {(ch,)}")
                rows = slice(ch, 2 * ch) if gate == "r" else slice(0, ch)
                kind = "q" if gate == "q" else "zr"
                getattr(self, f"w_{kind}_h{s}")[rows].copy_(w[:, :ch])
                getattr(self, f"w_{kind}_x{s}")[rows].copy_(w[:, ch:])
                getattr(self, f"b_{kind}{s}")[rows].copy_(b)

    @torch.no_grad()
    def reference_state_dict(self) -> dict:
        """The parameters under the reference module's keys and shapes, in its order, bit for bit: ``load_state_dict`` of the
        reference's ``SepConvGRU`` / ``ConvGRU`` takes it."""
        ch, out = self.hidden_dim, {}
        for s, _, _ in self.HALVES:
            for gate in "zrq":
                rows = slice(ch, 2 * ch) if gate == "r" else slice(0, ch)
                kind = "q" if gate == "q" else "zr"
                out[f"conv{gate}{s}.weight"] = torch.cat([getattr(self, f"w_{kind}_h{s}")[rows], getattr(self, f"w_{kind}_x{s}")[rows]], 1).clone()
                out[f"conv{gate}{s}.bias"] = getattr(self, f"b_{kind}{s}")[rows].clone()
        return out

    def forward(self, h: Tensor, x: Tensor) -> Tensor:
        """With ``hip_convs=True`` a call in which no gradient can be wanted — grad mode off, or neither ``h``, ``x`` nor a parameter
        requires grad — takes `fused_gru_half_inference` (the convolutions in HIP too); every other call, and every call of a module
        built with the default ``hip_convs=False``, takes `fused_gru_half`.  The two routes compute the same function up to float32
        summation order."""
        if torch.is_tensor(x):
            x = x.contiguous()
        half = fused_gru_half
        if self.hip_convs and not (torch.is_grad_enabled() and any(
                torch.is_tensor(t) and t.requires_grad for t in itertools.chain((h, x), self.parameters()))):
            half = fused_gru_half_inference
        for s, _, pad in self.HALVES:
            h = half(h, x, *(getattr(self, name + s) for name in ("w_zr_h", "w_zr_x", "b_zr", "w_q_h", "w_q_x", "b_q")), pad)
        return h


class FusedSepConvGRU(_FusedGRU):
    """GGRt's ``SepConvGRU`` (``ggrt/optimizer.py:51-78``): a horizontal 1×5 half-step, then a vertical 5×1 one, each four torch
    convolutions and two HIP launches.  Parameters per half (suffix 1, 2): ``w_zr_h``, ``w_zr_x``, ``b_zr``,
    ``w_q_h``, ``w_q_x``, ``b_q``.  ``forward(h, x)`` as the reference's; checkpoints move both ways through
    ``load_reference_state_dict`` / ``reference_state_dict``.  ``hip_convs=True`` (keyword only; a checkpoint does not know it): calls
    that need no gradient run their convolutions in HIP as well, two launches per half-step."""
    HALVES = (("1", (1, 5), (0, 2)), ("2", (5, 1), (2, 0)))


class FusedConvGRU(_FusedGRU):
    """GGRt's ``ConvGRU`` (``ggrt/optimizer.py:33-48``): one 3×3 step, as `FusedSepConvGRU` (parameters without a suffix)."""
    HALVES = (("", (3, 3), (1, 1)),)


def boundary_arguments(extrinsics, intrinsics, near, far, image_shape, background_color, gaussian_means,
                       gaussian_covariances, gaussian_sh_coefficients, gaussian_opacities, scale_invariant=True,
                       use_sh=True, gaussian_scales=None, gaussian_rotations=None, scissor=None, sh_max_degree=None,
                       antialiasing=False, return_alpha=False, *, return_projection=False, hits_grad=False, return_hits=0,
                       return_picks=False, return_contributions=False):
    """Everything ``render_cuda`` hands to the rasterizer, batched: a list of
    (GaussianRasterizationSettings, kwargs) per view.  Split out so the golden-vector tests can
    compare it with what the reference's call site produces.

    ``gaussian_covariances=None`` selects the fused-adapter form (§8f-4): ``gaussian_scales[b,g,3]`` +
    world-space ``gaussian_rotations[b,g,4]`` (w,x,y,z) go to the rasterizer's ``scales``/``rotations``
    inputs; the scale-invariant renormalisation then multiplies the scales by 1/near (≡ cov × 1/near²).

    ``antialiasing=True``: upstream's anti-aliased rasterization (``GaussianRasterizationSettings.antialiasing``) — off by
    default, as GGRt's checkpoints were trained."""
    assert use_sh or gaussian_sh_coefficients.shape[-1] == 1
    fused_adapter = gaussian_covariances is None
    if fused_adapter and (gaussian_scales is None or gaussian_rotations is None):
        raise ValueError("pass gaussian_covariances, or gaussian_scales together with gaussian_rotations")
    if scale_invariant:
        scale = 1 / near
        extrinsics = extrinsics.clone()
        extrinsics[..., :3, 3] = extrinsics[..., :3, 3] * scale[:, None]
        if fused_adapter:
            gaussian_scales = gaussian_scales * scale[:, None, None]
        else:
            gaussian_covariances = gaussian_covariances * (scale[:, None, None, None] ** 2)
        gaussian_means = gaussian_means * scale[:, None, None]
        near = near * scale
        far = far * scale
    d_sh = gaussian_sh_coefficients.shape[-1]
    degree = isqrt(d_sh) - 1
    shs = gaussian_sh_coefficients.permute(0, 1, 3, 2).contiguous()  # [b, g, d_sh, 3]
    b = extrinsics.shape[0]
    h, w = image_shape
    fov = get_fov(intrinsics)
    tan_half = (0.5 * fov).tan()
    tan_host = tan_half.detach().cpu().tolist()  # ONE device→host copy for the whole batch
    proj = get_projection_matrix(near, far, fov[:, 0], fov[:, 1], intrinsics).transpose(1, 2)
    view = torch.linalg.inv(extrinsics).transpose(1, 2)
    full = view @ proj
    if not fused_adapter:
        cov6 = torch.stack([gaussian_covariances[:, :, i, j] for i, j in _TRIU], dim=-1)  # [b, g, 6]
    out = []
    for i in range(b):
        settings = GaussianRasterizationSettings(
            image_height=h, image_width=w, tanfovx=tan_host[i][0], tanfovy=tan_host[i][1],
            bg=background_color[i], scale_modifier=1.0, viewmatrix=view[i], projmatrix=full[i],
            sh_degree=degree, campos=extrinsics[i, :3, 3], prefiltered=False,
            sh_max_degree=resolve_sh_max_degree(sh_max_degree), **({} if scissor is None else {"scissor": tuple(scissor)}),
            **({"antialiasing": True} if antialiasing else {}), **({"return_alpha": True} if return_alpha else {}),
            **({"return_contributions": True} if return_contributions else {}),
            **({"return_picks": True} if return_picks else {}), **({"return_hits": return_hits} if return_hits else {}), **({"hits_grad": True} if hits_grad else {}),
            **({"return_projection": True} if return_projection else {}))
        kwargs = dict(means3D=gaussian_means[i], shs=shs[i] if use_sh else None,
                      colors_precomp=None if use_sh else shs[i, :, 0, :],
                      opacities=gaussian_opacities[i, ..., None])
        if fused_adapter:
            kwargs.update(scales=gaussian_scales[i], rotations=gaussian_rotations[i])
        else:
            kwargs.update(cov3D_precomp=cov6[i])
        out.append((settings, kwargs))
    return out


def _rasterize_views(calls, aux=None, features=None):
    """Runs the per-view rasterizer calls of a batch, serially like the reference's loop
    (``cuda_splatting.py:93-127``) but without its two ``.item()`` syncs per view.

    (measured and dropped in round 1: spreading the views over HIP streams gained nothing —
    4 views at 480×352: 2.79 ms serial vs 2.87 ms on 4 streams, 3.44 ms with one host thread per stream —
    because at GGRt's sizes a view is host-bound (≈ 270 µs of launches + the `num_rendered` read-back per
    forward); the multi-stream autograd path also needed stream-lifetime care that is not worth carrying for
    no gain.  The lever is a sync-free forward with fewer launches, NOTES.md (old §8).)"""
    outs = []
    for i, (settings, kw) in enumerate(calls):
        mean_gradients = torch.zeros_like(kw["means3D"], requires_grad=True)  # the `means2D` gradient sink
        extra = {} if aux is None else {"aux_precomp": aux[i]}
        if features is not None:   # K more channels over the same lists: the call's tuple grows by features [K,h,w], last
            extra["features_precomp"] = features[i]
        outs.append(GaussianRasterizer(settings)(means2D=mean_gradients, **kw, **extra))
    return outs


def _stack_picks(ps) -> PixelPicks:
    """Per-call `PixelPicks` ([h,w] or [v,h,w] planes) → one with a leading axis over the calls"""
    return PixelPicks(*(torch.stack([getattr(p, f) for p in ps]) for f in PixelPicks._fields))


def _stack_hits(hs) -> PixelHits:
    """Per-call `PixelHits` → one with a leading axis over the calls"""
    return PixelHits(*(torch.stack([getattr(p, f) for p in hs]) for f in PixelHits._fields))


def _stack_projections(ps) -> Projection:
    """Per-call `Projection` → one with a leading axis over the calls"""
    return Projection(*(torch.stack([getattr(p, f) for p in ps]) for f in Projection._fields))


def _split_projection(out, want: bool):
    """(a rasterizer call's tuple without its `Projection`, the `Projection` or None): with `return_projection` it is the call's
    very last element, and everything in front of it sits where it sits without the setting"""
    return (out[:-1], out[-1]) if want else (out, None)


def _tail_index(want_contrib: bool, want_picks: bool, want_hits: bool = False):
    """Where a rasterizer call's tuple has (the rendered features, the Contributions): the hits, when on, are its last
    element, the picks, when on, stand in front of them (`_pick_index`), the contributions in front of those, the features in
    front of all three"""
    back = int(bool(want_picks)) + int(bool(want_hits))
    return -1 - int(bool(want_contrib)) - back, -1 - back


def _pick_index(want_hits: bool) -> int:
    """Where a rasterizer call's tuple has the PixelPicks: last, or in front of the PixelHits"""
    return -1 - int(bool(want_hits))


def _stack_contributions(cs) -> Contributions:
    """Per-call `Contributions` ([g] or [v,g] tensors) → one with a leading axis over the calls"""
    return Contributions(*(torch.stack([getattr(c, f) for c in cs]) for f in Contributions._fields))


def render_cuda(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape, background_color: Tensor,
                gaussian_means: Tensor, gaussian_covariances: Tensor, gaussian_sh_coefficients: Tensor,
                gaussian_opacities: Tensor, scale_invariant: bool = True, use_sh: bool = True,
                gaussian_scales: Optional[Tensor] = None, gaussian_rotations: Optional[Tensor] = None,
                scissor=None, sh_max_degree: Optional[int] = None, antialiasing: bool = False, return_alpha: bool = False,
                gaussian_features: Optional[Tensor] = None, *, return_projection: bool = False, hits_grad: bool = False,
                return_hits: int = 0, return_picks: bool = False, return_contributions: bool = False):
    """[batch] views → [batch,3,h,w] (reference ``cuda_splatting.py:49-128``).  With
    ``gaussian_covariances=None`` the ellipsoids come as scales + world quaternions (§8f-4).

    ``scissor=(x0, y0, x1, y1)`` (extension): render only the tiles overlapping that pixel window — for the
    fine-tune loop's deferred back-propagation (``finetune_ggrt_stable.py:126-142``), which renders the whole frame
    per crop cell and slices one cell out.  Inside the window the image equals the full render bit for bit.

    ``antialiasing=True`` (upstream's setting): opacities compensated for the screen-space dilation (``boundary_arguments``).

    ``return_alpha=True`` (extension): returns ``(color [batch,3,h,w], alpha [batch,h,w])``, alpha = 1 − T the accumulated
    opacity of the same pass, differentiable.

    ``gaussian_features [batch,g,K]`` (extension, 1 <= K <= 32): K per-Gaussian channels composited in one pass over the same
    lists; the result becomes a tuple whose LAST element is ``features [batch,K,h,w]`` (Σ f·α·T, no background).

    ``return_contributions=True`` (extension): the result becomes a tuple that ends — behind alpha and features — with a
    ``Contributions`` of ``[batch,g]`` tensors: per view and Gaussian Σ w, max w and the pixel count of the same pass.

    ``return_picks=True`` (extension; keyword-only): the tuple's VERY LAST element is a ``PixelPicks`` of ``[batch,h,w]``
    planes: per pixel the median depth / index, the dominant weight / index and the contributor count of the same pass.

    ``return_hits=K`` (extension; keyword-only, 1 <= K <= 32): a ``PixelHits`` behind even that — ``index`` / ``weight``
    ``[batch,K,h,w]``, ``rest`` / ``count`` ``[batch,h,w]``: per pixel the first K composited Gaussians of the same pass.
    ``hits_grad=True`` (keyword-only; needs ``return_hits``): its ``weight`` and ``rest`` are differentiable
    (``GaussianRasterizationSettings.hits_grad``).  The other render functions and ``DecoderSplattingCUDA.forward`` take the
    same keyword.

    ``return_projection=True`` (extension; keyword-only): a ``Projection`` of ``[batch,g,…]`` rows behind everything else — per
    view and Gaussian the 2D mean, depth value, conic, opacity, colour and ``valid``, differentiable
    (``GaussianRasterizationSettings.return_projection``).  The other render functions and ``DecoderSplattingCUDA.forward``
    take the same keyword (``DecoderOutput.projection``: ``[b,v,g,…]``)."""
    calls = boundary_arguments(extrinsics, intrinsics, near, far, image_shape, background_color, gaussian_means,
                               gaussian_covariances, gaussian_sh_coefficients, gaussian_opacities, scale_invariant,
                               use_sh, gaussian_scales, gaussian_rotations, scissor, sh_max_degree, antialiasing,
                               return_alpha, return_picks=return_picks, return_contributions=return_contributions,
                               return_hits=return_hits, hits_grad=hits_grad, return_projection=return_projection)
    outs = _rasterize_views(calls, features=gaussian_features)
    outs, projs = zip(*(_split_projection(o, return_projection) for o in outs)) if outs else ((), ())
    fi, ci = _tail_index(return_contributions, return_picks, return_hits)
    pi = _pick_index(return_hits)
    res = (torch.stack([o[0] for o in outs]),)
    if return_alpha:
        res += (torch.stack([o[3] for o in outs]),)
    if gaussian_features is not None:
        res += (torch.stack([o[fi] for o in outs]),)
    if return_contributions:
        res += (_stack_contributions([o[ci] for o in outs]),)
    if return_picks:
        res += (_stack_picks([o[pi] for o in outs]),)
    if return_hits:
        res += (_stack_hits([o[-1] for o in outs]),)
    if return_projection:
        res += (_stack_projections(projs),)
    return res if len(res) > 1 else res[0]


def depth_to_relative_disparity(depth, near, far, eps: float = 1e-10):
    """0 at near, 1 at far (reference ``encoder/epipolar/conversions.py:17-27``)."""
    disp_near, disp_far, disp = 1 / (near + eps), 1 / (far + eps), 1 / (depth + eps)
    return 1 - (disp - disp_far) / (disp_near - disp_far + eps)


def depth_feature(extrinsics: Tensor, gaussian_means: Tensor, near: Tensor, far: Tensor, mode: DepthRenderingMode):
    """Camera-space z of every Gaussian, mapped as reference ``cuda_splatting.py:240-252`` maps it."""
    w2c = torch.linalg.inv(extrinsics)
    z = (gaussian_means @ w2c[:, 2, :3, None]).squeeze(-1) + w2c[:, 2, 3, None]
    if mode == "disparity":
        z = 1 / z
    elif mode == "relative_disparity":
        z = depth_to_relative_disparity(z, near[:, None], far[:, None])
    elif mode == "log":
        z = z.minimum(near[:, None]).maximum(far[:, None]).log()
    return z


def render_depth_cuda(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape,
                      gaussian_means: Tensor, gaussian_covariances: Tensor, gaussian_opacities: Tensor,
                      scale_invariant: bool = True, mode: DepthRenderingMode = "depth", antialiasing: bool = False) -> Tensor:
    """Depth as colour, black background, channel mean → [batch,h,w] (reference ``cuda_splatting.py:227-269``)."""
    fake_color = depth_feature(extrinsics, gaussian_means, near, far, mode)
    b = fake_color.shape[0]
    result = render_cuda(extrinsics, intrinsics, near, far, image_shape,
                         torch.zeros((b, 3), dtype=fake_color.dtype, device=fake_color.device), gaussian_means,
                         gaussian_covariances, fake_color[:, :, None, None].expand(-1, -1, 3, 1), gaussian_opacities,
                         scale_invariant=scale_invariant, antialiasing=antialiasing)
    return result.mean(dim=1)


SH_C0 = 0.28209479177387814


def render_color_and_depth(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape,
                           background_color: Tensor, gaussian_means: Tensor, gaussian_covariances: Tensor,
                           gaussian_sh_coefficients: Tensor, gaussian_opacities: Tensor,
                           depth_mode: DepthRenderingMode = "depth", scale_invariant: bool = True,
                           use_sh: bool = True, gaussian_scales: Optional[Tensor] = None,
                           gaussian_rotations: Optional[Tensor] = None, sh_max_degree: Optional[int] = None,
                           antialiasing: bool = False, return_alpha: bool = False,
                           gaussian_features: Optional[Tensor] = None, *, return_projection: bool = False, hits_grad: bool = False,
                           return_hits: int = 0, return_picks: bool = False, return_contributions: bool = False):
    """ONE rasterization per view for what the reference obtains from two:
    ``render_cuda`` (colour, :49-128) + ``render_depth_cuda`` (:227-269).

    The reference's depth pass re-runs preprocess + sort + blend with the depth feature as a degree-0 SH
    coefficient, i.e. every Gaussian contributes ``max(0.5 + C0·f(z), 0)`` per channel over a black
    background, and the three identical channels are averaged.  Here that per-Gaussian value is handed to
    the rasterizer as its 4th blended feature (``aux_precomp``), so the depth image is the aux image of the
    SAME pass: identical values and gradients, half the work.  Returns ([b,3,h,w], [b,h,w]) — and the accumulated opacity
    [b,h,w] of the same pass as a third result with ``return_alpha=True``; with ``gaussian_features [b,g,K]`` the rendered
    ``features [b,K,h,w]`` of the same pass as the LAST result; with ``return_contributions=True`` a ``Contributions`` of
    ``[b,g]`` tensors behind everything else — except a ``PixelPicks`` of ``[b,h,w]`` planes, the very last result with
    ``return_picks=True`` (keyword-only; its ``median_depth`` holds the depth pass's per-Gaussian value ``max(0.5 + C0·f(z), 0)``)
    — and, with ``return_hits=K`` (keyword-only), a ``PixelHits`` (``[b,K,h,w]`` / ``[b,h,w]``) behind even that; with
    ``return_projection=True`` (keyword-only) a ``Projection`` of ``[b,g,…]`` rows last of all (its ``depth`` holds the depth
    pass's per-Gaussian value)."""
    feat = depth_feature(extrinsics, gaussian_means, near, far, depth_mode)  # unscaled, as the reference
    aux = (0.5 + SH_C0 * feat).clamp(min=0.0)
    calls = boundary_arguments(extrinsics, intrinsics, near, far, image_shape, background_color, gaussian_means,
                               gaussian_covariances, gaussian_sh_coefficients, gaussian_opacities, scale_invariant,
                               use_sh, gaussian_scales, gaussian_rotations, None, sh_max_degree, antialiasing, return_alpha,
                               return_picks=return_picks, return_contributions=return_contributions, return_hits=return_hits, hits_grad=hits_grad,
                               return_projection=return_projection)
    outs = _rasterize_views(calls, aux=aux, features=gaussian_features)
    outs, projs = zip(*(_split_projection(o, return_projection) for o in outs)) if outs else ((), ())
    fi, ci = _tail_index(return_contributions, return_picks, return_hits)
    pi = _pick_index(return_hits)
    planes = (0, 2, 3) if return_alpha else (0, 2)
    if gaussian_features is not None:
        planes += (fi,)
    res = tuple(torch.stack([o[k] for o in outs]) for k in planes)
    if return_contributions:
        res += (_stack_contributions([o[ci] for o in outs]),)
    if return_picks:
        res += (_stack_picks([o[pi] for o in outs]),)
    if return_hits:
        res += (_stack_hits([o[-1] for o in outs]),)
    return res + (_stack_projections(projs),) if return_projection else res


def render_views_fused(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape,
                       background_color: Tensor, gaussians: Gaussians, view_to_batch,
                       depth_mode: Optional[DepthRenderingMode] = None, scale_invariant: bool = True,
                       device_camera: bool = True, list_capacity: int = 0, batched: bool = True, scissor=None,
                       sh_max_degree: Optional[int] = None, antialiasing: bool = False, return_alpha: bool = False,
                       gaussian_features: Optional[Tensor] = None, *, return_projection: bool = False, hits_grad: bool = False,
                       return_hits: int = 0, return_picks: bool = False, return_contributions: bool = False):
    """The call site with NO torch operation on a Gaussian-sized tensor (SURVEY.md §8 a2 "where time goes"):

    * ``device_camera``: view / projection matrices, camera position, tan(fov/2) and 1/near of all views come
      from one library kernel and stay on the device (no ``.item()`` / ``.cpu()`` — reference :104-105);
      with ``list_capacity > 0`` (sync-free forward) the whole call then runs without any host sync;
    * the Gaussians are not repeated per view (reference ``decoder_splatting_cuda.py:47-50``): view n reads
      batch element ``view_to_batch[n]`` of ``gaussians`` directly;
    * the 1/near renormalisation of means and covariances (``cuda_splatting.py:66-73``) travels as a device
      scalar (``input_scale``) and is applied when the kernel loads them;
    * ``harmonics`` stay ``[g,3,d_sh]`` (``sh_channel_major``) — no transpose copy (:77) and no copy back in
      backward; ``covariances`` stay ``[g,3,3]`` — the upper-triangle gather (:116,124) happens on load;
    * ``depth_mode="depth"``: the depth-as-colour feature ``max(0.5 + C0·z, 0)`` (:240-269) is formed inside the
      kernel from the view depth (``aux_affine``); the other modes still build it with torch.

    * ``batched``: the views that share a batch element go through ONE launch set (``rasterize_views``, SURVEY.md
      §8f-2): the Gaussians are read once for all of them, one depth sort, one tile-list build, one blend launch,
      gradients summed over the views inside the backward kernel — instead of one rasterizer call per view and
      autograd adding the per-view gradient tensors.  A batch element with a single view takes the per-view call.

    Same images and gradients as ``render_color_and_depth`` / ``render_cuda`` up to fp32 rounding
    (``tests/test_callsite_fused.py``).  extrinsics/intrinsics/near/far/background: one row per view.
    Returns (color [n,3,h,w], depth [n,h,w] | None) — with ``return_alpha=True`` also alpha [n,h,w], the accumulated
    opacity 1 − T of the same launches (differentiable); with ``gaussian_features [b,g,K]`` (one feature set per batch
    element, shared by its views) also ``features [n,K,h,w]``, rendered through the same launch sets, as the LAST result;
    with ``return_contributions=True`` a ``Contributions`` of ``[n,g]`` tensors (per view and Gaussian Σ w, max w, pixel
    count of the same launch sets; not differentiable) behind everything else — except, with ``return_picks=True`` (keyword-only),
    a ``PixelPicks`` of ``[n,h,w]`` planes (per pixel the median depth / index, the dominant weight / index and the contributor
    count of the same launch sets; indices within the view's batch element; not differentiable), the very last result — but for
    ``return_hits=K`` (keyword-only, 1 <= K <= 32), which puts a ``PixelHits`` behind it: ``index`` / ``weight`` ``[n,K,h,w]``,
    ``rest`` / ``count`` ``[n,h,w]``, per pixel the first K composited Gaussians of the same launch sets (not differentiable).
    ``return_projection=True`` (keyword-only): a ``Projection`` of ``[n,g,…]`` rows (per view and Gaussian of its batch element the
    2D mean, depth value, conic, opacity, colour and ``valid``; differentiable) last of all."""
    n = extrinsics.shape[0]
    has_feat = gaussian_features is not None
    want_proj = bool(return_projection)
    want_contrib, want_picks, n_hits = bool(return_contributions), bool(return_picks), int(return_hits)
    fi, ci = _tail_index(want_contrib, want_picks, n_hits)   # where a rasterizer call's tuple has the rendered features / contributions
    pi = _pick_index(n_hits)                                  # … and the picks
    h, w = image_shape
    d_sh = gaussians.harmonics.shape[-1]
    degree = isqrt(d_sh) - 1
    sh_cap = resolve_sh_max_degree(sh_max_degree)
    ext_orig = extrinsics
    # the per-view camera quantities: one library kernel, everything (incl. tan(fov/2) and 1/near) stays on the
    # device — poses / intrinsics that carry gradients included (camera_setup is differentiable: one more launch in the
    # backward, and the rasterizer returns dL/dtan(fov/2)) — or, for CPU golden tests, the reference's torch formulation
    on_device = device_camera and extrinsics.is_cuda
    if on_device:
        from .rasterizer import camera_setup
        view, full, campos, tanfov, scale = camera_setup(extrinsics, intrinsics, near, far, scale_invariant)
        tan_host = None
        if not scale_invariant:
            scale = None
    else:
        if scale_invariant:
            scale = 1 / near
            extrinsics = extrinsics.clone()
            extrinsics[..., :3, 3] = extrinsics[..., :3, 3] * scale[:, None]
            near_s, far_s = near * scale, far * scale
        else:
            scale, near_s, far_s = None, near, far
        fov = get_fov(intrinsics)
        tan_half = (0.5 * fov).tan()
        tan_host = tan_half.detach().cpu().tolist()
        proj = get_projection_matrix(near_s, far_s, fov[:, 0], fov[:, 1], intrinsics).transpose(1, 2)
        view = torch.linalg.inv(extrinsics).transpose(1, 2)
        full = view @ proj
        # (on the GPU tan(fov/2) goes on as a tensor, so that this branch too gives intrinsics their whole gradient)
        campos, tanfov = extrinsics[:, :3, 3], (tan_half.float().contiguous() if extrinsics.is_cuda else None)
    fused_cov = gaussians.covariances is not None
    # ---- every batch element in ONE launch set (GgrViews.num_sets): the reference's `(b v)` flattening with
    # per-batch-element Gaussians (decoder_splatting_cuda.py:40-60) without its per-view loop, its v× repeat, or a
    # Python loop over batch elements — view n renders Gaussian set n // v of the [b, g, …] tensors as they are
    nb = gaussians.means.shape[0]
    vpb = n // nb if nb and n % nb == 0 else 0
    if (batched and nb > 1 and vpb >= 1 and extrinsics.is_cuda and nb <= 64 and
            list(int(x) for x in view_to_batch) == [i // vpb for i in range(n)]):
        from .rasterizer import rasterize_views
        aux, aux_affine = None, None
        if depth_mode == "depth":
            aux_affine = (0.5, SH_C0)
        elif depth_mode is not None:
            feat = depth_feature(ext_orig, gaussians.means.repeat_interleave(vpb, 0), near, far, depth_mode)  # [n, g]
            aux = (0.5 + SH_C0 * feat).clamp(min=0.0)
        tf = tanfov if tanfov is not None else torch.tensor(tan_host, dtype=torch.float32, device=view.device)
        settings = GaussianRasterizationSettings(
            image_height=h, image_width=w, tanfovx=0.0, tanfovy=0.0, bg=background_color[0], scale_modifier=1.0,
            viewmatrix=view[0], projmatrix=full[0], sh_degree=degree, campos=campos[0], prefiltered=False,
            list_capacity=list_capacity * n, sh_channel_major=True, aux_affine=aux_affine,
            sh_max_degree=sh_cap, scissor=None if scissor is None else tuple(scissor), antialiasing=bool(antialiasing),
            return_alpha=bool(return_alpha), return_contributions=want_contrib, return_picks=want_picks, return_hits=n_hits, hits_grad=bool(hits_grad),
            return_projection=want_proj)
        kw = dict(cov3D_precomp=gaussians.covariances) if fused_cov else dict(scales=gaussians.scales,
                                                                              rotations=gaussians.rotations)
        out = rasterize_views(gaussians.means, gaussians.opacities, view, full, campos, background_color, tf,
                              settings, shs=gaussians.harmonics, aux_precomp=aux, input_scale=scale,
                              features_precomp=gaussian_features, **kw)
        out, pj = _split_projection(out, want_proj)
        return _fused_result(out[0], out[2] if depth_mode is not None else None, out[3] if return_alpha else None,
                             return_alpha, out[fi] if has_feat else None, out[ci] if want_contrib else None,
                                 out[pi] if want_picks else None, out[-1] if n_hits else None, pj)
    # batch element b of every Gaussian tensor WITHOUT `t[b]`: select's backward zero-fills a full [B,…] tensor
    # and copies the slice in, per view (0.2 ms per view for 1 M × 25 SH coefficients).  One unbind per tensor
    # (backward = one stack) — or a free reshape when there is a single batch element, GGRt's case.
    def per_batch(t: Optional[Tensor]):
        if t is None:
            return None
        return [t.reshape(t.shape[1:])] if t.shape[0] == 1 else list(t.unbind(0))
    g_means, g_cov, g_sh, g_op = (per_batch(gaussians.means), per_batch(gaussians.covariances),
                                  per_batch(gaussians.harmonics), per_batch(gaussians.opacities))
    g_scales, g_rot, g_feat = per_batch(gaussians.scales), per_batch(gaussians.rotations), per_batch(gaussian_features)
    colors, depths, alphas, feats, contribs, picks = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
    hits, projs = [None] * n, [None] * n
    groups = {}
    for i in range(n):
        groups.setdefault(int(view_to_batch[i]), []).append(i)
    single = []
    for b, idx in groups.items():
        if not (batched and len(idx) > 1 and extrinsics.is_cuda):
            single += idx
            continue
        # ---- all views of batch element b in one launch set ----
        from .rasterizer import rasterize_views
        ii = torch.as_tensor(idx, device=view.device)
        contiguous = idx == list(range(idx[0], idx[0] + len(idx)))
        take = (lambda t: t[idx[0]:idx[0] + len(idx)]) if contiguous else (lambda t: t.index_select(0, ii))
        aux, aux_affine = None, None
        if depth_mode == "depth":
            aux_affine = (0.5, SH_C0)
        elif depth_mode is not None:  # per-Gaussian feature per view, built with torch: [V,P]
            feat = depth_feature(take(ext_orig), g_means[b][None].expand(len(idx), -1, -1), take(near), take(far), depth_mode)
            aux = (0.5 + SH_C0 * feat).clamp(min=0.0)
        tf = take(tanfov) if tanfov is not None else torch.tensor([tan_host[i] for i in idx], dtype=torch.float32,
                                                                  device=view.device)
        settings = GaussianRasterizationSettings(
            image_height=h, image_width=w, tanfovx=0.0, tanfovy=0.0, bg=background_color[idx[0]], scale_modifier=1.0,
            viewmatrix=view[idx[0]], projmatrix=full[idx[0]], sh_degree=degree, campos=campos[idx[0]],
            prefiltered=False, list_capacity=list_capacity * len(idx), sh_channel_major=True, aux_affine=aux_affine,
            sh_max_degree=sh_cap, scissor=None if scissor is None else tuple(scissor), antialiasing=bool(antialiasing),
            return_alpha=bool(return_alpha), return_contributions=want_contrib, return_picks=want_picks, return_hits=n_hits, hits_grad=bool(hits_grad),
            return_projection=want_proj)
        kw = dict(cov3D_precomp=g_cov[b]) if fused_cov else dict(scales=g_scales[b], rotations=g_rot[b])
        out = rasterize_views(g_means[b], g_op[b][..., None], take(view), take(full), take(campos),
                              take(background_color), tf, settings, shs=g_sh[b], aux_precomp=aux,
                              input_scale=None if scale is None else take(scale),
                              features_precomp=g_feat[b] if has_feat else None, **kw)
        out, pj = _split_projection(out, want_proj)
        col, dep = out[0], out[2]
        if len(idx) == n and contiguous:  # every view in this one launch set: hand its outputs on as they are
            return _fused_result(col, dep if depth_mode is not None else None, out[3] if return_alpha else None,
                                 return_alpha, out[fi] if has_feat else None, out[ci] if want_contrib else None,
                                 out[pi] if want_picks else None, out[-1] if n_hits else None, pj)
        for k, i in enumerate(idx):
            colors[i], depths[i] = col[k], dep[k]
            if want_proj:
                projs[i] = Projection(*(t[k] for t in pj))
            if has_feat:
                feats[i] = out[fi][k]
            if want_contrib:
                contribs[i] = Contributions(*(t[k] for t in out[ci]))
            if want_picks:
                picks[i] = PixelPicks(*(t[k] for t in out[pi]))
            if n_hits:
                hits[i] = PixelHits(*(t[k] for t in out[-1]))
            if return_alpha:
                alphas[i] = out[3][k]
    for i in single:
        b = int(view_to_batch[i])
        aux, aux_affine = None, None
        if depth_mode == "depth":
            aux_affine = (0.5, SH_C0)
        elif depth_mode is not None:  # disparity / relative_disparity / log: per-Gaussian feature built with torch
            feat = depth_feature(ext_orig[i:i + 1], g_means[b][None], near[i:i + 1], far[i:i + 1], depth_mode)
            aux = (0.5 + SH_C0 * feat[0]).clamp(min=0.0)
        settings = GaussianRasterizationSettings(
            image_height=h, image_width=w, tanfovx=tan_host[i][0] if tan_host else 0.0,
            tanfovy=tan_host[i][1] if tan_host else 0.0, bg=background_color[i],
            scale_modifier=1.0, viewmatrix=view[i], projmatrix=full[i], sh_degree=degree,
            campos=campos[i], prefiltered=False, list_capacity=list_capacity,
            input_scale=None if scale is None else scale[i:i + 1], sh_channel_major=True, aux_affine=aux_affine,
            tanfov=None if tanfov is None else tanfov[i], sh_max_degree=sh_cap,
            scissor=None if scissor is None else tuple(scissor), antialiasing=bool(antialiasing),
            return_alpha=bool(return_alpha), return_contributions=want_contrib, return_picks=want_picks, return_hits=n_hits, hits_grad=bool(hits_grad),
            return_projection=want_proj)
        means = g_means[b]
        kw = dict(cov3D_precomp=g_cov[b]) if fused_cov else dict(scales=g_scales[b], rotations=g_rot[b])
        # means2D is only a gradient sink (`cuda_splatting.py:95-99`): its values are never read
        sink = torch.empty_like(means).requires_grad_()
        out = GaussianRasterizer(settings)(means3D=means, means2D=sink, opacities=g_op[b][..., None], shs=g_sh[b],
                                           aux_precomp=aux, features_precomp=g_feat[b] if has_feat else None, **kw)
        out, projs[i] = _split_projection(out, want_proj)
        colors[i], depths[i] = out[0], out[2]
        if has_feat:
            feats[i] = out[fi]
        if want_contrib:
            contribs[i] = out[ci]
        if want_picks:
            picks[i] = out[pi]
        if n_hits:
            hits[i] = out[-1]
        if return_alpha:
            alphas[i] = out[3]
    # one view (GGRt's usual call): a view of the rasterizer's output instead of a stack — no copy kernel forward,
    # none backward
    stack = lambda ts: ts[0].unsqueeze(0) if len(ts) == 1 else torch.stack(ts)
    return _fused_result(stack(colors), stack(depths) if depth_mode is not None else None,
                         stack(alphas) if return_alpha else None, return_alpha, stack(feats) if has_feat else None,
                         _stack_contributions(contribs) if want_contrib else None, _stack_picks(picks) if want_picks else None,
                         _stack_hits(hits) if n_hits else None, _stack_projections(projs) if want_proj else None)


def _fused_result(color, depth, alpha, return_alpha, features=None, contributions=None, picks=None, hits=None, projection=None):
    """render_views_fused's result: (color, depth) as always, (color, depth, alpha) with return_alpha; the rendered feature
    channels, when asked for, come behind them, the contributions, when asked for, behind those, then the picks, the hits, and
    the projection last"""
    res = (color, depth, alpha) if return_alpha else (color, depth)
    if features is not None:
        res += (features,)
    if contributions is not None:
        res += (contributions,)
    if picks is not None:
        res += (picks,)
    if hits is not None:
        res += (hits,)
    return res if projection is None else res + (projection,)


def contribution_keep_mask(contributions: Contributions, min_weight_max: Optional[float] = None,
                           min_pixel_count: Optional[int] = None) -> Tensor:
    """Which Gaussians to KEEP, from the `Contributions` of one or more views: boolean ``[b,g]`` for ``[b,v,g]`` tensors
    (``DecoderOutput.contributions``), ``[g]`` for ``[v,g]`` (``rasterize_views``) — and for ``[g]`` tensors as they are.
    The view axis is reduced with ``amax``: a Gaussian stays if ANY view gives it a blend weight of at least
    ``min_weight_max`` (RadSplat's criterion) and, when given as well, sees it on at least ``min_pixel_count`` pixels.  With
    neither threshold: the Gaussians that were composited anywhere at all (``pixel_count > 0`` in some view)."""
    wmax, count = contributions.weight_max, contributions.pixel_count
    if wmax.dim() >= 2:
        wmax, count = wmax.amax(dim=-2), count.amax(dim=-2)
    if min_weight_max is None and min_pixel_count is None:
        return count > 0
    keep = torch.ones_like(count, dtype=torch.bool)
    if min_weight_max is not None:
        keep &= wmax >= min_weight_max
    if min_pixel_count is not None:
        keep &= count >= min_pixel_count
    return keep


class DecoderSplattingCUDA(nn.Module):
    """Same call contract as reference ``decoder_splatting_cuda.py:19-85``:
    ``forward(gaussians, extrinsics[b,v,4,4], intrinsics[b,v,3,3], near[b,v], far[b,v], image_shape,
    depth_mode) -> DecoderOutput(color[b,v,3,h,w], depth[b,v,h,w] | None)``; with ``return_alpha=True`` (extension) the
    output's ``alpha[b,v,h,w]`` holds the accumulated opacity 1 − T of the colour pass, differentiable."""

    def __init__(self, cfg=None, fused_depth: bool = True, fused_inputs: bool = True, list_capacity: int = 0,
                 sh_max_degree: Optional[int] = None, antialiasing: bool = False):
        super().__init__()
        self.cfg = cfg
        # upstream's anti-aliased rasterization (GaussianRasterizationSettings.antialiasing) for every render of this decoder;
        # False (default): as GGRt's checkpoints were trained
        self.antialiasing = bool(antialiasing)
        # 3 / 4: the explicit choice of INTEGRATION.md §7, for THIS decoder (two decoders of one process may differ); None =
        # this layer's default at the time of each call (set_sh_max_degree / GGR_SH_MAX_DEGREE)
        self.sh_max_degree = None if sh_max_degree is None else resolve_sh_max_degree(sh_max_degree)
        # > 0: sync-free rasterizer forward with per-tile lists of at most this many entries — with the fused
        # inputs the whole decoder call then has no host sync and can be captured in a HIP graph
        # (check ``ggrt_official_amd.last_forward_status()`` for overflow when a sync is affordable)
        self.list_capacity = int(list_capacity)
        self.fused_depth = fused_depth  # False: two rasterizations per view, literally as the reference
        self.fused_inputs = fused_inputs  # False: the reference's torch pre-processing of the Gaussian tensors
        self.register_buffer("background_color", torch.zeros(3, dtype=torch.float32), persistent=False)

    @staticmethod
    def _per_view(t: Tensor, v: int) -> Tensor:
        """[b, ...] → [(b v), ...] (every view sees the same Gaussians; the rasterizer only reads them)."""
        return t[:, None].expand(-1, v, *t.shape[1:]).reshape(-1, *t.shape[1:])

    @classmethod
    def _opt_per_view(cls, t: Optional[Tensor], v: int) -> Optional[Tensor]:
        return None if t is None else cls._per_view(t, v)

    @classmethod
    def _ellipsoids(cls, gaussians: Gaussians, v: int) -> dict:
        if gaussians.covariances is not None:
            return {}
        return dict(gaussian_scales=cls._per_view(gaussians.scales, v),
                    gaussian_rotations=cls._per_view(gaussians.rotations, v))

    def forward(self, gaussians: Gaussians, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                image_shape, depth_mode: Optional[DepthRenderingMode] = None, scissor=None,
                return_alpha: bool = False, gaussian_features: Optional[Tensor] = None,
                *, return_projection: bool = False, hits_grad: bool = False, return_hits: int = 0, return_picks: bool = False,
                return_contributions: bool = False) -> DecoderOutput:
        """``scissor=(x0, y0, x1, y1)`` (extension, fused path): render only that pixel window's tiles — the
        deferred-backprop cell of ``finetune_ggrt_stable.py:126-142``.  ``return_alpha=True`` (extension): the output's
        ``alpha`` [b,v,h,w] is the accumulated opacity of the colour pass; colour and depth are as without it.
        ``gaussian_features`` [b,g,K] (extension, 1 <= K <= 32): the output's ``features`` [b,v,K,h,w] holds those per-Gaussian
        channels composited through the colour pass's own launch set (Σ f·α·T, no background), differentiable.
        ``return_contributions=True`` (extension): the output's ``contributions`` holds [b,v,g] tensors — per view and
        Gaussian Σ w, max w and the pixel count of the colour pass (``contribution_keep_mask`` turns them into a pruning mask).
        ``return_picks=True`` (extension; keyword-only): the output's ``picks`` holds [b,v,h,w] planes — per pixel the median depth
        and its Gaussian, the dominant blend weight and its Gaussian (indices within the batch element's g Gaussians, −1 where
        nothing was composited) and the contributor count of the colour pass; not differentiable (``pick_values``).
        ``return_hits=K`` (extension; keyword-only, 1 <= K <= 32): the output's ``hits`` holds ``index`` / ``weight`` [b,v,K,h,w]
        and ``rest`` / ``count`` [b,v,h,w] — per pixel the first K Gaussians the colour pass composited, front to back, with
        their blend weights; not differentiable (``composite_hits``, per view).
        ``return_projection=True`` (extension; keyword-only): the output's ``projection`` holds [b,v,g,…] rows — per view and
        Gaussian the 2D mean, depth value, conic, opacity, colour and ``valid`` of the colour pass, differentiable."""
        b, v = extrinsics.shape[:2]
        want_proj = bool(return_projection)
        unflat_j = lambda pj: None if pj is None else Projection(*(t.reshape(b, v, *t.shape[1:]) for t in pj))
        alpha = None
        has_feat = gaussian_features is not None
        want_contrib, want_picks, n_hits = bool(return_contributions), bool(return_picks), int(return_hits)
        fi, ci = _tail_index(want_contrib, want_picks, n_hits)
        pi = _pick_index(n_hits)
        unflat = lambda t: t.reshape(b, v, *t.shape[1:])
        unflat_c = lambda out: Contributions(*(unflat(t) for t in out[ci])) if want_contrib else None
        unflat_p = lambda out: PixelPicks(*(unflat(t) for t in out[pi])) if want_picks else None
        unflat_h = lambda out: PixelHits(*(unflat(t) for t in out[-1])) if n_hits else None
        if scissor is not None and not (self.fused_inputs and self.fused_depth):
            raise ValueError("scissor needs the fused call site (fused_inputs and fused_depth)")
        bg = self.background_color.to(far.device)[None].expand(b * v, 3)
        if self.fused_inputs and self.fused_depth:
            # no per-view copies of the Gaussians, no torch op on a Gaussian-sized tensor (render_views_fused)
            out = render_views_fused(
                extrinsics.flatten(0, 1), intrinsics.flatten(0, 1), near.flatten(), far.flatten(), image_shape, bg,
                gaussians, [n // v for n in range(b * v)], depth_mode, list_capacity=self.list_capacity,
                scissor=scissor, sh_max_degree=self.sh_max_degree, antialiasing=self.antialiasing, return_alpha=return_alpha,
                gaussian_features=gaussian_features, return_contributions=want_contrib, return_picks=want_picks, return_hits=n_hits, hits_grad=bool(hits_grad),
                return_projection=want_proj)
            out, pj = _split_projection(out, want_proj)
            color, depth = out[0], out[1]
            if return_alpha:
                alpha = out[2].reshape(b, v, *out[2].shape[1:])
            return DecoderOutput(color.reshape(b, v, *color.shape[1:]),
                                 None if depth is None else depth.reshape(b, v, *depth.shape[1:]), alpha,
                                 unflat(out[fi]) if has_feat else None, unflat_c(out), unflat_p(out), unflat_h(out), unflat_j(pj))
        if depth_mode is not None and self.fused_depth:
            out = render_color_and_depth(
                extrinsics.flatten(0, 1), intrinsics.flatten(0, 1), near.flatten(), far.flatten(), image_shape, bg,
                self._per_view(gaussians.means, v), self._opt_per_view(gaussians.covariances, v),
                self._per_view(gaussians.harmonics, v), self._per_view(gaussians.opacities, v), depth_mode,
                sh_max_degree=self.sh_max_degree, antialiasing=self.antialiasing, return_alpha=return_alpha,
                gaussian_features=self._opt_per_view(gaussian_features, v), return_contributions=want_contrib,
                return_picks=want_picks, return_hits=n_hits, hits_grad=hits_grad, return_projection=want_proj,
                **self._ellipsoids(gaussians, v))
            out, pj = _split_projection(out, want_proj)
            color, depth = out[0], out[1]
            if return_alpha:
                alpha = out[2].reshape(b, v, *out[2].shape[1:])
            return DecoderOutput(color.reshape(b, v, *color.shape[1:]), depth.reshape(b, v, *depth.shape[1:]), alpha,
                                 unflat(out[fi]) if has_feat else None, unflat_c(out), unflat_p(out), unflat_h(out), unflat_j(pj))
        color = render_cuda(extrinsics.flatten(0, 1), intrinsics.flatten(0, 1), near.flatten(), far.flatten(),
                            image_shape, bg, self._per_view(gaussians.means, v),
                            self._opt_per_view(gaussians.covariances, v), self._per_view(gaussians.harmonics, v),
                            self._per_view(gaussians.opacities, v), sh_max_degree=self.sh_max_degree,
                            antialiasing=self.antialiasing, return_alpha=return_alpha,
                            gaussian_features=self._opt_per_view(gaussian_features, v), return_contributions=want_contrib,
                            return_picks=want_picks, return_hits=n_hits, hits_grad=hits_grad, return_projection=want_proj,
                            **self._ellipsoids(gaussians, v))
        features, contributions, picks, hits, pj = None, None, None, None, None
        if want_proj:   # (the very last element; what is left is the result without it)
            color, pj = (color[:-1] if len(color) > 2 else color[0]), color[-1]
        if n_hits:   # (the last element; what is left is the result without it)
            color, hits = (color[:-1] if len(color) > 2 else color[0]), PixelHits(*(unflat(t) for t in color[-1]))
        if want_picks:   # (then the picks)
            color, picks = (color[:-1] if len(color) > 2 else color[0]), PixelPicks(*(unflat(t) for t in color[-1]))
        if want_contrib:   # (then the contributions)
            color, contributions = (color[:-1] if len(color) > 2 else color[0]), Contributions(*(unflat(t) for t in color[-1]))
        if has_feat:
            color, features = color[:-1] if return_alpha else color[0], unflat(color[-1])
        if return_alpha:   # (the colour pass's; the reference's separate depth pass below has its own)
            color, alpha = color
            alpha = alpha.reshape(b, v, *alpha.shape[1:])
        color = color.reshape(b, v, *color.shape[1:])
        depth = None if depth_mode is None else self.render_depth(gaussians, extrinsics, intrinsics, near, far,
                                                                  image_shape, depth_mode)
        return DecoderOutput(color, depth, alpha, features, contributions, picks, hits, unflat_j(pj))

    def render_depth(self, gaussians: Gaussians, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                     image_shape, mode: DepthRenderingMode = "depth") -> Tensor:
        b, v = extrinsics.shape[:2]
        result = render_depth_cuda(extrinsics.flatten(0, 1), intrinsics.flatten(0, 1), near.flatten(), far.flatten(),
                                   image_shape, self._per_view(gaussians.means, v),
                                   self._per_view(gaussians.covariances, v), self._per_view(gaussians.opacities, v),
                                   mode=mode, antialiasing=self.antialiasing)
        return result.reshape(b, v, *result.shape[1:])
