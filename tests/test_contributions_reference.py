"""The contribution reference (tests/contributions_reference.py) against the frozen oracle — no GPU.

weight_sum is the oracle's own d(Σ colour)/d rgb[:,0] with bg = 0 (autograd through `tr.blend`: the colour's channel 0 is
Σ w·rgb[:,0], so its gradient w.r.t. rgb[g,0] is Σ_pixels w of Gaussian g); per pixel the weights add up to 1 − final_T; and
pixel_count equals a brute-force loop over the pixels of a 32×32 frame.  Both legs run in float64: agreement is to rounding."""
import numpy as np
import pytest
import torch

from ggrt_official_amd.synthetic import make_scene
from oracle import torch_raster as tr
from tests import contributions_reference as cr

CASES = [(1500, 83, 45, True, False, 911), (1200, 64, 48, False, True, 912)]   # P, W, H, use_cov, antialiasing, seed


def _lists(sc, use_cov, aa):
    d = lambda t: t.double()
    kw = dict(cov3D_precomp=d(sc.cov3D)) if use_cov else dict(scales=d(sc.scales), rotations=d(sc.rotations))
    return cr.lists(d(sc.means3D), d(sc.opacities), d(sc.viewmatrix), d(sc.projmatrix), d(sc.campos), sc.width, sc.height,
                    sc.tanfovx, sc.tanfovy, sc.sh_degree, shs=d(sc.shs), sh_cap=3, antialiasing=aa, **kw)


@pytest.mark.parametrize("P,W,H,use_cov,aa,seed", CASES)
def test_weight_sum_is_the_oracles_colour_gradient_and_weights_add_up_to_the_opacity(P, W, H, use_cov, aa, seed):
    sc = make_scene(P, W, H, sh_degree=1, seed=seed)
    pre, point_list, ranges = _lists(sc, use_cov, aa)
    wsum, wmax, count, acc = cr.reduce_lists(pre, point_list, ranges, W, H, per_pixel=True)
    rgb = pre["rgb"].detach().clone().requires_grad_(True)
    p2 = dict(pre)
    p2["rgb"] = rgb
    color, final_T, _n, _d = tr.blend(p2, point_list, ranges, torch.zeros(3, dtype=torch.float64), W, H, want_depth=False)
    color.sum().backward()
    assert float(wsum.max()) > 0.5 and int((count > 0).sum()) > P // 10
    assert torch.allclose(wsum, rgb.grad[:, 0], rtol=1e-12, atol=1e-14)
    assert torch.allclose(acc, 1.0 - final_T, rtol=0, atol=1e-12)
    assert bool(((count > 0) == (wmax > 0)).all()) and bool((wmax <= wsum + 1e-15).all()) and float(wmax.max()) <= 0.99
    assert bool((wsum <= wmax * count.double() * (1 + 1e-12)).all())
    assert not bool(count[pre["radii"] == 0].any())


def test_pixel_count_equals_a_brute_force_loop_over_the_pixels():
    W = H = 32
    sc = make_scene(400, W, H, sh_degree=0, seed=913)
    pre, point_list, ranges = _lists(sc, True, False)
    _, wmax, count = cr.reduce_lists(pre, point_list, ranges, W, H)
    xy, con, op = pre["xy"].numpy(), pre["conic"].numpy(), pre["opacity"].numpy()
    want, want_max = np.zeros(400, np.int64), np.zeros(400)
    gx = (W + 15) // 16
    for y in range(H):
        for x in range(W):
            r0, r1 = (int(v) for v in ranges[(y // 16) * gx + x // 16])
            T = 1.0
            for g in point_list[r0:r1].tolist():
                dx, dy = xy[g, 0] - x, xy[g, 1] - y
                power = -0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) - con[g, 1] * dx * dy
                if power > 0:
                    continue
                alpha = min(0.99, op[g] * np.exp(power))
                if alpha < 1.0 / 255.0:
                    continue
                if T * (1 - alpha) < 1e-4:
                    break
                want[g] += 1
                want_max[g] = max(want_max[g], alpha * T)
                T *= 1 - alpha
    assert want.sum() > 1000
    assert np.array_equal(count.numpy(), want)
    assert np.allclose(wmax.numpy(), want_max, rtol=1e-12, atol=0)
