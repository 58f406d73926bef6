"""The pick reference (tests/picks_reference.py) — no GPU.

1. On a tiny scene it equals a naive per-pixel Python loop over the tile's list (the compositing rule written out).
2. The condition check of the GPU test's reference scenes (tests/test_gpu_picks.py, picks_reference.REF_CASES): the reference
   computed in float32 and in float64 agrees on median_index, max_index and count in EVERY pixel and on max_weight within
   helpers.FWD_ATOL, so the caps of the GPU comparison are not used up by the reference's own rounding.  Seeds were tried in
   order from 981 per scene and the first that passed was committed: A 981, B 981 (measured: 0 differing pixels, max
   |Δ max_weight| 1.1e-6 and 4.0e-7).  Each scene also has a tile whose list exceeds two full staging batches (512 entries;
   measured 1950 and 2560 with the oracle's rects) and pixels that stop before their list ends (every covered pixel does)."""
import numpy as np
import pytest
import torch

from ggrt_official_amd.synthetic import make_scene
from tests import contributions_reference as cr
from tests import picks_reference as pr
from tests.helpers import FWD_ATOL


def test_reference_equals_a_naive_loop_over_the_pixels():
    W, H, P = 40, 24, 200
    sc = make_scene(P, W, H, sh_degree=0, seed=982)
    d = lambda t: t.double()
    pre, point_list, ranges = cr.lists(d(sc.means3D), d(sc.opacities), d(sc.viewmatrix), d(sc.projmatrix), d(sc.campos), W, H,
                                       sc.tanfovx, sc.tanfovy, 0, shs=d(sc.shs), cov3D_precomp=d(sc.cov3D) * 0.02, sh_cap=3)   # (small
    # Gaussians: some pixels stay empty)
    got = pr.pick_planes(pre, point_list, ranges, W, H)
    xy, con, op, dep = pre["xy"].numpy(), pre["conic"].numpy(), pre["opacity"].numpy(), pre["depth"].numpy()
    med_i, max_i = np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    med_d, max_w, count = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
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
                if T > 0.5:
                    med_i[y, x], med_d[y, x] = g, dep[g]
                if alpha * T > max_w[y, x]:
                    max_i[y, x], max_w[y, x] = g, alpha * T
                count[y, x] += 1
                T *= 1 - alpha
    assert count.sum() > 1000 and (count == 0).any() and (med_i != max_i).sum() > 20
    assert np.array_equal(got["median_index"].numpy(), med_i) and np.array_equal(got["max_index"].numpy(), max_i)
    assert np.array_equal(got["count"].numpy(), count)
    assert np.array_equal(got["median_depth"].numpy(), med_d)
    assert np.allclose(got["max_weight"].numpy(), max_w, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", list(pr.REF_CASES))
def test_reference_scenes_are_well_conditioned_and_reach_the_long_paths(name):
    _sc, _colors, r64 = pr.ref_case(name, torch.float64)
    _sc, _colors, r32 = pr.ref_case(name, torch.float32)
    H, W = r64["count"].shape
    for k in ("median_index", "max_index", "count"):
        assert torch.equal(r32[k], r64[k]), f"{name}: the float32 and float64 references differ in {k}"
    dw = float((r32["max_weight"].double() - r64["max_weight"]).abs().max())
    print(f"{name}: max |Δ max_weight| between the float32 and float64 references {dw:.3e}")
    assert dw <= FWD_ATOL
    assert r64["longest"] > 512, "no tile list of more than two staging batches"
    assert r64["stopped"] >= 1, "no pixel stops before its list ends"
    assert int((r64["count"] > 0).sum()) > W * H // 2 and int((r64["median_index"] != r64["max_index"]).sum()) > 100
