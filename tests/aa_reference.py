"""Anti-aliased torch reference, COMPOSED from the frozen `oracle.torch_raster` (which has no anti-aliasing of its own).

Upstream's `antialiasing` setting (Mip-Splatting's 2D filter) scales each Gaussian's opacity by
s = sqrt(max(2.5e-5, det(Σ2D) / det(Σ2D + 0.3·I))).  Here the dilated (a, b, c) are recovered by inverting the oracle's
conic, the opacity is multiplied by s, and the oracle's own binning and blend run on the result; autograd differentiates
the whole chain (conic, means, covariance, camera)."""
import torch

from oracle import torch_raster as tr

AA_MIN_RATIO = 2.5e-5


def aa_scale(conic):
    """s per Gaussian from the oracle's conic (c/det, −b/det, a/det) of the DILATED 2D covariance."""
    c0, c1, c2 = conic.unbind(-1)
    dc = c0 * c2 - c1 * c1
    dc = torch.where(dc != 0, dc, torch.ones_like(dc))
    a, b, c = c2 / dc, -c1 / dc, c0 / dc
    det1 = a * c - b * b
    det1 = torch.where(det1 != 0, det1, torch.ones_like(det1))
    det0 = (a - tr.DILATION) * (c - tr.DILATION) - b * b
    return torch.sqrt(torch.clamp(det0 / det1, min=AA_MIN_RATIO))


def rasterize_aa(means3D, opacities, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, sh_degree=0,
                 shs=None, colors_precomp=None, cov3D_precomp=None, scales=None, rotations=None, sh_cap=None,
                 antialiasing=True):
    """(color [3,H,W], radii [P], depth [H,W], pre) of the oracle with the anti-aliased opacity."""
    pre = tr.preprocess(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree, shs,
                        colors_precomp, cov3D_precomp, scales, rotations, sh_cap=sh_cap)
    if antialiasing:
        pre = dict(pre)
        pre["opacity_raw"] = pre["opacity"]
        pre["aa_scale"] = aa_scale(pre["conic"])
        pre["opacity"] = pre["opacity"] * pre["aa_scale"]
    point_list, ranges, _keys, _n = tr.bin_tiles(pre, W, H)
    color, _final_T, _n_contrib, depth = tr.blend(pre, point_list, ranges, bg, W, H)
    return color, pre["radii"].to(torch.int32), depth, pre
