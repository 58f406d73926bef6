"""The hit reference (tests/hits_reference.py) and `composite_hits` — no GPU.

1. On a tiny scene the reference equals a naive per-pixel Python loop over the tile's list (the compositing rule written out).
2. The condition check of the GPU test's reference scenes (tests/test_gpu_hits.py, hits_reference.REF_CASES at K = REF_K): the
   reference computed in float32 and in float64 agrees on EVERY slot index and EVERY count (0 differing pixels) and on the
   weights and the rest within helpers.FWD_ATOL, so the cap of the GPU comparison is not used up by the reference's own rounding.
   The pick tests' two scenes satisfy it with their seeds as they are (981, 981), the third scene (small Gaussians: most pixels
   do not fill their K slots) with the first seed tried (992).  Measured: 0 differing pixels in all three; max |Δ weight|
   1.2e-6, 6.1e-7, 7.4e-6; max |Δ rest| 1.1e-6, 6.0e-7, 1.1e-7.
3. The reference is consistent with the pick reference on the same lists: the same count, and — where count <= K — max_weight
   is the largest slot weight and max_index the earliest slot that holds it.
4. `composite_hits`: equal to a hand loop, differentiable in `values` (gradcheck in float64), raises on a wrong shape."""
import numpy as np
import pytest
import torch

import ggrt_official_amd as g
from ggrt_official_amd.synthetic import make_scene
from tests import contributions_reference as cr
from tests import hits_reference as hr
from tests import picks_reference as pr
from tests.helpers import FWD_ATOL


def test_reference_equals_a_naive_loop_over_the_pixels():
    W, H, P, K = 40, 24, 200, 3
    sc = make_scene(P, W, H, sh_degree=0, seed=982)
    d = lambda t: t.double()
    pre, point_list, ranges = cr.lists(d(sc.means3D), d(sc.opacities), d(sc.viewmatrix), d(sc.projmatrix), d(sc.campos), W, H,
                                       sc.tanfovx, sc.tanfovy, 0, shs=d(sc.shs), cov3D_precomp=d(sc.cov3D) * 0.02, sh_cap=3)   # (small
    # Gaussians: some pixels stay empty)
    got = hr.hit_arrays(pre, point_list, ranges, W, H, K)
    xy, con, op = pre["xy"].numpy(), pre["conic"].numpy(), pre["opacity"].numpy()
    index, weight = np.full((K, H, W), -1, np.int64), np.zeros((K, H, W))
    rest, count = np.zeros((H, W)), np.zeros((H, W), np.int64)
    gx = (W + 15) // 16
    for y in range(H):
        for x in range(W):
            r0, r1 = (int(v) for v in ranges[(y // 16) * gx + x // 16])
            T = 1.0
            for gid in point_list[r0:r1].tolist():
                dx, dy = xy[gid, 0] - x, xy[gid, 1] - y
                power = -0.5 * (con[gid, 0] * dx * dx + con[gid, 2] * dy * dy) - con[gid, 1] * dx * dy
                if power > 0:
                    continue
                alpha = min(0.99, op[gid] * np.exp(power))
                if alpha < 1.0 / 255.0:
                    continue
                if T * (1 - alpha) < 1e-4:
                    break
                if count[y, x] < K:
                    index[count[y, x], y, x], weight[count[y, x], y, x] = gid, alpha * T
                else:
                    rest[y, x] += alpha * T
                count[y, x] += 1
                T *= 1 - alpha
    assert count.sum() > 1000 and (count == 0).any() and (count > K).sum() > 50 and ((count > 0) & (count < K)).sum() > 50
    assert np.array_equal(got["index"].numpy(), index) and np.array_equal(got["count"].numpy(), count)
    assert np.allclose(got["weight"].numpy(), weight, rtol=1e-12, atol=0)
    assert np.allclose(got["rest"].numpy(), rest, rtol=1e-12, atol=1e-15)
    assert ((got["index"].numpy() >= 0).sum(0) == np.minimum(count, K)).all()


@pytest.mark.parametrize("name", list(hr.REF_CASES))
def test_reference_scenes_are_well_conditioned_and_consistent_with_the_pick_reference(name):
    K = hr.REF_K
    _sc, _colors, r64, p64 = hr.ref_case(name, torch.float64)
    _sc, _colors, r32, p32 = hr.ref_case(name, torch.float32)
    H, W = r64["count"].shape
    differing = (r32["index"] != r64["index"]).any(0) | (r32["count"] != r64["count"])
    dw = float((r32["weight"].double() - r64["weight"]).abs().max())
    dr = float((r32["rest"].double() - r64["rest"]).abs().max())
    few = r64["count"] <= K
    print(f"{name}: {int(differing.sum())} pixels differ between the float32 and float64 references; max |Δ weight| {dw:.3e}, "
          f"max |Δ rest| {dr:.3e}; {int(few.sum())} of {W * H} pixels with count <= K, largest count {int(r64['count'].max())}")
    assert int(differing.sum()) == 0
    assert dw <= FWD_ATOL and dr <= FWD_ATOL
    if name in hr.COV_SCALE:   # the slots are not filled: empty pixels, partly filled ones — and some that leave a rest all the same
        assert int((r64["count"] == 0).sum()) > 100 and int(((r64["count"] > 0) & (r64["count"] < K)).sum()) > 1000
        assert int((r64["count"] > K).sum()) >= 1
    else:                      # the slots are filled and leave a rest
        assert int((r64["count"] > K).sum()) > W * H // 2 and float(r64["rest"].max()) > 0.1
    assert torch.equal((r64["index"] >= 0).sum(0), r64["count"].clamp(max=K))
    assert bool((r64["rest"][few] == 0).all()) and bool((r64["weight"][r64["index"] < 0] == 0).all())
    # … and the pick reference, on the same lists, says the same
    for r, picks in ((r64, p64), (r32, p32)):
        assert torch.equal(r["count"], picks["count"])
        if name in hr.COV_SCALE:
            assert int(few.sum()) > 1000
            assert torch.equal(r["weight"].max(0).values[few], picks["max_weight"][few])
            first = (r["weight"] == r["weight"].max(0).values[None]).to(torch.int32).argmax(0)
            assert torch.equal(r["index"].gather(0, first[None])[0][few], picks["max_index"][few])


def _hits(K=3, H=4, W=5, P=6, seed=0):
    gen = torch.Generator().manual_seed(seed)
    index = torch.randint(-1, P, (K, H, W), generator=gen, dtype=torch.int32)
    weight = torch.rand(K, H, W, generator=gen)
    weight[index < 0] = 7.0                      # (a padding slot contributes nothing, whatever its weight says)
    return g.PixelHits(index, weight, torch.zeros(H, W), (index >= 0).sum(0).to(torch.int32))


def test_composite_hits_equals_a_hand_loop():
    hits = _hits()
    K, H, W = hits.index.shape
    for values in (torch.arange(6, dtype=torch.float32) * 0.5 + 1, torch.randn(6, 4, generator=torch.Generator().manual_seed(1))):
        out = g.composite_hits(values, hits)
        assert out.shape == (H, W) + tuple(values.shape[1:]) and out.dtype == values.dtype
        want = torch.zeros_like(out)
        for k in range(K):
            for y in range(H):
                for x in range(W):
                    i = int(hits.index[k, y, x])
                    if i >= 0:
                        want[y, x] += hits.weight[k, y, x] * values[i]
        assert torch.allclose(out, want, rtol=1e-6, atol=1e-6)
    empty = g.PixelHits(torch.full((2, 3, 3), -1, dtype=torch.int32), torch.zeros(2, 3, 3), torch.zeros(3, 3),
                        torch.zeros(3, 3, dtype=torch.int32))
    assert torch.equal(g.composite_hits(torch.ones(4), empty), torch.zeros(3, 3))


def test_composite_hits_is_differentiable_in_values_and_raises_on_a_wrong_shape():
    hits = _hits(seed=2)
    h64 = g.PixelHits(hits.index, hits.weight.double(), hits.rest.double(), hits.count)
    for shape in ((6,), (6, 2)):
        v = torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: g.composite_hits(t, h64), (v,))
    v = torch.ones(6, requires_grad=True)
    g.composite_hits(v, hits).sum().backward()
    want = torch.zeros(6).index_add_(0, hits.index[hits.index >= 0].long(), hits.weight[hits.index >= 0])
    assert torch.allclose(v.grad, want, rtol=1e-6, atol=1e-6)               # the weights of the slots that name the row
    with pytest.raises(ValueError):
        g.composite_hits(torch.zeros(2, 2, 2), hits)
    with pytest.raises(ValueError):
        g.composite_hits(torch.zeros(6), g.PixelHits(hits.index[0], hits.weight[0], hits.rest, hits.count))
    with pytest.raises(ValueError):
        g.composite_hits(torch.zeros(6), g.PixelHits(hits.index, hits.weight[:2], hits.rest, hits.count))
