"""Accumulated-opacity torch reference, COMPOSED from the frozen `oracle.torch_raster` (which returns no alpha of its own).

The oracle's colour is Σ c·α·T + T_final·bg, differentiable in T_final.  So for any channel k
    alpha = 1 − T_final = 1 − (colour_k with bg = 1 − colour_k with bg = 0),
two oracle blends over the same lists (the lists do not depend on bg); autograd differentiates the whole chain (means,
covariance, opacity, camera), with or without the anti-aliased opacity of tests/aa_reference.py."""
import torch

from oracle import torch_raster as tr
from tests.aa_reference import aa_scale


def rasterize_alpha(means3D, opacities, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, sh_degree=0,
                    shs=None, colors_precomp=None, cov3D_precomp=None, scales=None, rotations=None, sh_cap=None,
                    antialiasing=False):
    """(color [3,H,W], radii [P], depth [H,W], alpha [H,W]) of the oracle; alpha composed as above."""
    pre = tr.preprocess(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree, shs,
                        colors_precomp, cov3D_precomp, scales, rotations, sh_cap=sh_cap)
    if antialiasing:
        pre = dict(pre)
        pre["opacity"] = pre["opacity"] * aa_scale(pre["conic"])
    point_list, ranges, _keys, _n = tr.bin_tiles(pre, W, H)
    color, _final_T, _n_contrib, depth = tr.blend(pre, point_list, ranges, bg, W, H)
    dt = pre["xy"].dtype
    one, zero = torch.ones(3, dtype=dt), torch.zeros(3, dtype=dt)
    c1 = tr.blend(pre, point_list, ranges, one, W, H, want_depth=False)[0]
    c0 = tr.blend(pre, point_list, ranges, zero, W, H, want_depth=False)[0]
    alpha = 1.0 - (c1[0] - c0[0])
    return color, pre["radii"].to(torch.int32), depth, alpha
