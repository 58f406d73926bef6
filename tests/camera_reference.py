"""The call site's camera setup in float64 torch — view / projection matrices, camera position, tan(fov/2), 1/near — restated
from the torch branch of `splatting.render_views_fused` (`get_fov`, `get_projection_matrix`, the inverse): the oracle of
`camera_setup`'s backward (tests/test_gpu_intrinsics_grad.py), and, chained in front of `oracle.torch_raster`, the
reference of `intrinsics.grad` / `extrinsics.grad` end to end.  tests/test_intrinsics_grad_abi.py holds its forward to that
branch's values on the CPU.

Plain module, not a test file (like tests/camera_scenes.py)."""
from __future__ import annotations

import numpy as np
import torch


def fov_tan_half(intrinsics: torch.Tensor) -> torch.Tensor:
    """[n,3,3] normalised intrinsics → [n,2] tan(fov/2): half the angle between the rays through the mid-points of opposite
    image edges, each view from its OWN intrinsics"""
    inv = torch.linalg.inv(intrinsics)

    def ray(u, v):
        d = inv @ torch.tensor([u, v, 1.0], dtype=intrinsics.dtype)
        return d / d.norm(dim=-1, keepdim=True)

    fov_x = (ray(0.0, 0.5) * ray(1.0, 0.5)).sum(-1).acos()
    fov_y = (ray(0.5, 0.0) * ray(0.5, 1.0)).sum(-1).acos()
    return (0.5 * torch.stack((fov_x, fov_y), dim=-1)).tan()


def projection(near: torch.Tensor, far: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """GGRt's projection [n,4,4]: the X / Y rows from intrinsics[0] for EVERY view (the reference's quirk)"""
    n = near.shape[0]
    k0 = intrinsics[0]
    zero, one = torch.zeros(n, dtype=near.dtype), torch.ones(n, dtype=near.dtype)
    rows = [torch.stack([2 * near * k0[0, 0], zero, (2 * k0[0, 2] - 1) * one, zero], -1),
            torch.stack([zero, 2 * near * k0[1, 1], (2 * k0[1, 2] - 1) * one, zero], -1),
            torch.stack([zero, zero, far / (far - near), -(far * near) / (far - near)], -1),
            torch.stack([zero, zero, one, zero], -1)]
    return torch.stack(rows, 1)


def camera_setup_ref(extrinsics, intrinsics, near, far, scale_invariant=True):
    """(view [n,4,4], full [n,4,4], campos [n,3], tanfov [n,2], scale [n]) in float64; differentiable w.r.t. extrinsics and
    intrinsics (near / far are constants, as at the call site)"""
    e, k = extrinsics.double(), intrinsics.double()
    nr, fr = near.double().detach(), far.double().detach()
    if scale_invariant:
        scale = 1.0 / nr
        col = torch.cat([scale[:, None].expand(-1, 3), torch.ones_like(scale)[:, None]], -1)    # the translation · scale
        mult = torch.ones(e.shape[0], 4, 4, dtype=torch.float64)
        mult[:, :, 3] = col
        e = e * mult
        nr, fr = nr * scale, fr * scale
    else:
        scale = torch.ones_like(nr)
    view = torch.linalg.inv(e).transpose(1, 2)
    full = view @ projection(nr, fr, k).transpose(1, 2)
    return view, full, e[:, :3, 3], fov_tan_half(k), scale


def cameras(n, seed=0, W=64, H=48):
    """n views: rotated and translated poses, NON-SQUARE intrinsics (fx ≠ fy in normalised units beyond the frame's aspect)
    with an OFF-CENTRE principal point, each view its own, near / far each view its own: float32 (extrinsics, intrinsics,
    near, far)"""
    g = torch.Generator().manual_seed(1000 + seed)
    ext = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    for i in range(n):
        w = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.4
        K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        ext[i, :3, :3] = torch.matrix_exp(K)
        ext[i, :3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6
    intr = torch.eye(3, dtype=torch.float64).repeat(n, 1, 1)
    fx = 0.8 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)
    intr[:, 0, 0] = fx
    intr[:, 1, 1] = fx * (W / H) * (0.85 + 0.3 * torch.rand(n, generator=g, dtype=torch.float64))
    off = lambda: (0.02 + 0.06 * torch.rand(n, generator=g, dtype=torch.float64)) * (1 - 2 * (torch.rand(n, generator=g) < 0.5).double())
    intr[:, 0, 2] = 0.5 + off()     # 2 … 8 % of the frame off the centre, either side
    intr[:, 1, 2] = 0.5 + off()
    near = 0.7 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)
    far = 60.0 + 40.0 * torch.rand(n, generator=g, dtype=torch.float64)
    return ext.float(), intr.float(), near.float(), far.float()


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
