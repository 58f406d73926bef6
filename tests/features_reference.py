"""Feature-channel torch reference, COMPOSED from the frozen `oracle.torch_raster` (which blends three colour channels).

features [K,H,W] = Σ f_k·α·T: for each 3-channel slice of the per-Gaussian features the oracle's own `blend` runs with
`pre["rgb"]` replaced by the slice (zero-padded to three channels), bg = 0 and no depth, over the lists of ONE `preprocess` +
`bin_tiles`; autograd differentiates the whole chain (features, means, covariance, opacity, camera), with or without the
anti-aliased opacity of tests/aa_reference.py."""
import torch

from oracle import torch_raster as tr
from tests.aa_reference import aa_scale


def rasterize_features(means3D, opacities, features, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, sh_degree=0,
                       shs=None, colors_precomp=None, cov3D_precomp=None, scales=None, rotations=None, sh_cap=None,
                       antialiasing=False):
    """(color [3,H,W], radii [P], depth [H,W], features [K,H,W]) of the oracle; the features composed as above."""
    pre = tr.preprocess(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree, shs,
                        colors_precomp, cov3D_precomp, scales, rotations, sh_cap=sh_cap)
    if antialiasing:
        pre = dict(pre)
        pre["opacity"] = pre["opacity"] * aa_scale(pre["conic"])
    point_list, ranges, _keys, _n = tr.bin_tiles(pre, W, H)
    color, _final_T, _n_contrib, depth = tr.blend(pre, point_list, ranges, bg, W, H)
    dt = pre["xy"].dtype
    zero = torch.zeros(3, dtype=dt)
    K = features.shape[1]
    planes = []
    for k0 in range(0, K, 3):
        sl = features[:, k0:k0 + 3].to(dt)
        n = sl.shape[1]
        if n < 3:
            sl = torch.cat([sl, torch.zeros(sl.shape[0], 3 - n, dtype=dt)], dim=1)
        p2 = dict(pre)
        p2["rgb"] = sl
        planes.append(tr.blend(p2, point_list, ranges, zero, W, H, want_depth=False)[0][:n])
    return color, pre["radii"].to(torch.int32), depth, torch.cat(planes, dim=0)
