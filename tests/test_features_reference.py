"""The composed feature reference (tests/features_reference.py) against central finite differences, in float64, on the small
hand-placed scene the anti-aliasing reference was checked on (tests/test_antialiasing_abi.py `_scene64`: six Gaussians, none
near an α or T threshold) — the reference itself is checked here, on the CPU, before the GPU tests lean on it."""
import pytest
import torch

from oracle import torch_raster as tr
from tests.features_reference import rasterize_features
from tests.test_antialiasing_abi import _scene64

K = 5


def _inputs():
    W, H, tanx, tany, view, proj, means, cov, op, colors = _scene64()
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(means.shape[0], K, generator=g, dtype=torch.float64)
    wts = torch.randn(K, H, W, generator=g, dtype=torch.float64)
    return (W, H, tanx, tany, view, proj, colors, wts), dict(means3D=means, cov3D=cov, opacity=op, features=feats)


def _loss(fixed, x, aa):
    W, H, tanx, tany, view, proj, colors, wts = fixed
    z = torch.zeros(3, dtype=torch.float64)
    out = rasterize_features(x["means3D"], x["opacity"], x["features"], view, proj, z, z, W, H, tanx, tany,
                             colors_precomp=colors, cov3D_precomp=x["cov3D"], antialiasing=aa)
    return (out[3] * wts).sum(), out


def test_feature_planes_are_the_colour_blend_of_their_slices():
    fixed, x = _inputs()
    W, H, tanx, tany, view, proj, colors, wts = fixed
    _, out = _loss(fixed, x, False)
    planes = out[3]
    assert planes.shape == (K, H, W) and float(planes.abs().max()) > 0
    z = torch.zeros(3, dtype=torch.float64)
    col = tr.rasterize(x["means3D"], x["opacity"], view, proj, z, z, W, H, tanx, tany, 0, colors_precomp=x["features"][:, :3],
                       cov3D_precomp=x["cov3D"])[0]
    assert torch.equal(col, planes[:3])   # channels 0..2 as colours over black ARE the colour image
    # a channel scaled by a constant scales its plane; the last slice (two channels) is padded, not wrapped
    x2 = dict(x, features=x["features"] * torch.tensor([1.0, 1.0, 1.0, 2.0, 1.0], dtype=torch.float64))
    p2 = _loss(fixed, x2, False)[1][3]
    torch.testing.assert_close(p2[3], 2.0 * planes[3])
    assert torch.equal(p2[4], planes[4])


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("which", ["means3D", "cov3D", "opacity", "features"])
def test_composed_reference_gradients_match_finite_differences(which, aa):
    fixed, base = _inputs()
    leaves = {k: v.clone().requires_grad_() for k, v in base.items()}
    loss, _ = _loss(fixed, leaves, aa)
    loss.backward()
    g = leaves[which].grad
    x = base[which]
    eps = {"means3D": 1e-6, "cov3D": 1e-9, "opacity": 1e-6, "features": 1e-4}[which]
    checked = 0
    for gi in range(x.shape[0]):
        for k in range(x.shape[1]):
            if which == "cov3D" and gi == 4:
                continue   # (the clamp-regime Gaussian's covariance is 1e-11: a step of 1e-9 leaves its regime)
            xp, xm = x.clone(), x.clone()
            xp[gi, k] += eps
            xm[gi, k] -= eps
            lp, _ = _loss(fixed, dict(base, **{which: xp}), aa)
            lm, _ = _loss(fixed, dict(base, **{which: xm}), aa)
            fd = float((lp - lm) / (2 * eps))
            an = float(g[gi, k])
            # (the bar of the anti-aliasing reference's check)
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 1e-4 * abs(an), (which, gi, k, fd, an)
            checked += 1
    assert checked >= 6
