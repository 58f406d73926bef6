"""Self-checks of tests/hits_grad_reference.py (no GPU).

1. The closed form the kernel implements, on a hand-built list of 3 entries at one pixel, K = 2, a gradient on both slots and on
   the rest: autograd through the reference gives dL/dα_i = T_i·g_i − S_i/(1−α_i).
2. Central finite differences in float64 on a 16×16 frame of a few Gaussians.
3. The condition check of the GPU test's reference scenes: at K = 1, 8 and 32 the reference computed in float32 and in float64
   agrees on EVERY slot index and EVERY count, so that the GPU test may demand the same of the GPU.
4. The differentiable arrays equal tests/hits_reference.py's detached ones."""
import numpy as np
import pytest
import torch

from tests import distortion_reference as dr
from tests import hits_grad_reference as hg
from tests import hits_reference as hr


def _one_pixel(alphas):
    """`pre` of len(alphas) Gaussians centred on pixel (0, 0) of a 1×1 frame: α at the pixel is the opacity"""
    n = len(alphas)
    op = torch.tensor(alphas, dtype=torch.float64, requires_grad=True)
    pre = dict(xy=torch.zeros(n, 2, dtype=torch.float64), conic=torch.tensor([[1.0, 0.0, 1.0]] * n, dtype=torch.float64), opacity=op)
    return pre, op, torch.arange(n, dtype=torch.int32), torch.tensor([[0, n]])


def test_closed_form_on_three_entries_two_slots():
    alphas, K = [0.5, 0.25, 0.4], 2
    pre, op, point_list, ranges = _one_pixel(alphas)
    arr = hg.hit_arrays(pre, point_list, ranges, 1, 1, K)
    assert arr["index"].reshape(-1).tolist() == [0, 1] and int(arr["count"]) == 3
    T = [1.0, 0.5, 0.375]
    assert torch.allclose(arr["weight"].reshape(-1), torch.tensor([0.5, 0.25 * 0.5], dtype=torch.float64))
    assert torch.allclose(arr["rest"].reshape(-1), torch.tensor([0.4 * 0.375], dtype=torch.float64))
    g0, g1, gr = 0.7, -1.3, 2.1
    loss = g0 * arr["weight"][0, 0, 0] + g1 * arr["weight"][1, 0, 0] + gr * arr["rest"][0, 0]
    loss.backward()
    want = hg.closed_form_dalpha(torch.tensor(alphas, dtype=torch.float64), torch.tensor([g0, g1, gr], dtype=torch.float64))
    assert torch.allclose(op.grad, want, rtol=1e-12, atol=1e-14), (op.grad, want)
    # … and by hand: w = (.5, .125, .15); S_0 = g1·w1 + gr·w2, S_1 = gr·w2, S_2 = 0
    w = [0.5, 0.125, 0.15]
    hand = [T[0] * g0 - (g1 * w[1] + gr * w[2]) / 0.5, T[1] * g1 - gr * w[2] / 0.75, T[2] * gr]
    assert np.allclose(op.grad.numpy(), hand, rtol=1e-12)


def test_closed_form_with_a_capped_a_skipped_and_a_stop_entry():
    """the cap passes the gradient straight through (as distortion_reference.tile_weights); a skipped entry (α < 1/255) and the
    stop entry (T·(1−α) < 1e-4) get nothing and take no slot"""
    alphas, K = [0.995, 0.001, 0.98, 0.97, 0.9], 2     # capped to .99 | skipped | T: .01 → 2e-4 | stop: 2e-4·.03 < 1e-4 | dead
    pre, op, point_list, ranges = _one_pixel(alphas)
    arr = hg.hit_arrays(pre, point_list, ranges, 1, 1, K)
    assert arr["index"].reshape(-1).tolist() == [0, 2] and int(arr["count"]) == 2 and float(arr["rest"].detach()) == 0.0
    g0, g1 = 0.6, -0.9
    (g0 * arr["weight"][0, 0, 0] + g1 * arr["weight"][1, 0, 0] + 5.0 * arr["rest"][0, 0]).backward()
    want = hg.closed_form_dalpha(torch.tensor([0.99, 0.98], dtype=torch.float64), torch.tensor([g0, g1], dtype=torch.float64))
    assert torch.allclose(op.grad[[0, 2]], want, rtol=1e-12) and not op.grad[[1, 3, 4]].any()


def test_reference_equals_central_finite_differences():
    from ggrt_official_amd.synthetic import make_scene
    W = H = 16
    K = 2
    sc = make_scene(6, W, H, sh_degree=0, seed=7)
    G = torch.randn(K, H, W, generator=torch.Generator().manual_seed(71), dtype=torch.float64)
    Gr = torch.randn(H, W, generator=torch.Generator().manual_seed(72), dtype=torch.float64)

    def run(kw):
        pre, point_list, ranges = hg.preprocess_lists(kw, sc)
        arr = hg.hit_arrays(pre, point_list, ranges, W, H, K)
        return (arr["weight"] * G).sum() + (arr["rest"] * Gr).sum(), arr

    kw = dr.scene_inputs(sc, torch.float64, leaf=True)
    loss, arr = run(kw)
    assert int(arr["count"].max()) > K and int((arr["count"] > 0).sum()) > 20, "the frame must fill slots and the rest"
    loss.backward()
    eps = 1e-6
    for i, name in enumerate(("means3D", "opacities", "cov3D_precomp", "viewmatrix", "projmatrix")):
        d = torch.randn(kw[name].shape, generator=torch.Generator().manual_seed(80 + i), dtype=torch.float64)
        d = d * kw[name].detach().abs().mean(-1, keepdim=True)   # (relative to each row: the covariances span two decades)
        vals = []
        for sgn in (1.0, -1.0):
            moved = {k: v.detach() for k, v in kw.items()}
            moved[name] = moved[name] + sgn * eps * d
            with torch.no_grad():
                l, a = run(moved)
            assert torch.equal(a["index"], arr["index"]) and torch.equal(a["count"], arr["count"]), "a discrete decision moved"
            vals.append(float(l))
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = float((kw[name].grad * d).sum())
        print(f"{name}: finite difference {fd:.9e}, autograd {an:.9e}")
        assert abs(an) > 0 and abs(fd - an) <= 1e-6 * abs(an) + 1e-9, name


@pytest.mark.parametrize("name", list(hg.REF_CASES))
def test_reference_scenes_are_well_conditioned_at_every_k(name):
    """float32 and float64 agree on every index and every count at K = 1, 8, 32 (0 differing pixels): the GPU test may demand
    equality in every pixel.  The arrays also equal hits_reference's (detached) ones."""
    _P, W, H, _D, use_sh, use_cov, aa, _seed = hg.REF_CASES[name]
    sc, colors = hg.ref_scene(name)
    graphs = {}
    for dt in (torch.float32, torch.float64):
        with torch.no_grad():
            pre, point_list, ranges = hr.scene_lists(sc, use_sh, use_cov, colors, aa, dt)
            graphs[dt] = (pre, point_list, ranges, hg.tile_graph(pre, point_list, ranges, W, H))
    for K in hg.REF_KS:
        a32, a64 = (hg.hit_arrays(*graphs[dt][:3], W, H, K, graphs[dt][3]) for dt in (torch.float32, torch.float64))
        differing = (a32["index"] != a64["index"]).any(0) | (a32["count"] != a64["count"])
        print(f"{name} K={K}: {int(differing.sum())} pixels differ between the float32 and float64 references; "
              f"count max {int(a64['count'].max())}, pixels with count > K {int((a64['count'] > K).sum())}, "
              f"with count < K {int((a64['count'] < K).sum())}")
        assert not bool(differing.any())
        if K == hr.REF_K:
            old = hr.ref_case(name, torch.float64)[2]
            assert torch.equal(old["index"], a64["index"]) and torch.equal(old["count"], a64["count"])
            assert torch.allclose(old["weight"], a64["weight"], rtol=1e-12, atol=0) and torch.allclose(old["rest"], a64["rest"], rtol=1e-10, atol=1e-300)


def test_the_shared_graph_gives_gradients_for_every_input():
    name = "C_small_gaussians_unfilled_slots"
    _P, W, H = hg.REF_CASES[name][:3]
    G = torch.randn(8, H, W, generator=torch.Generator().manual_seed(5))
    Gr = torch.randn(H, W, generator=torch.Generator().manual_seed(6))
    both = hg.ref_grads(name, 8, G, Gr)
    gw, gr = hg.ref_grads(name, 8, G, None), hg.ref_grads(name, 8, None, Gr)
    for k in ("means3D", "opacities", "cov3D_precomp", "viewmatrix", "projmatrix"):
        assert np.abs(both[k]).max() > 0 and np.allclose(both[k], gw[k] + gr[k], rtol=1e-9, atol=1e-12), k
    assert not np.any(both["shs"]) and not np.any(both["campos"])   # the weights do not depend on the colours
