"""tests/absgrad_reference.py pinned, on the CPU, before anything is compared with it.

* Its planes are `tr.blend`'s, and its SIGNED sums are the frozen oracle's autograd gradient of the loss w.r.t. `pre["xy"]`
  times (½W, ½H): rel-L2 ≤ 1e-10 in float64, for a colour loss and for colour + depth + alpha.
* absgrad ≥ |signed| elementwise.
* The CONDITION the GPU comparison rests on (tests/test_gpu_absgrad.py): on its scene, under its upstream gradients, at least
  half of the composited Gaussians have absgrad_x > 1.5·|signed_x| — a kernel that returned the signed sums could not pass.
  `clustered_scene()`'s default seed (1301) satisfies it: measured, 77 … 79 % of the ≈ 324 composited Gaussians in every form
  (the upstream gradients are white noise, so the per-pixel terms of most footprints change sign).
* The rounding floor: the reference's own float32 run against its float64 run.  Measured on the GPU scene (rel-L2 over all rows):
      form a (colour only)              absgrad 1.8e-7   signed 5.5e-7
      form b (colour + depth + alpha)   absgrad 9.9e-8   signed 7.3e-7
      form c (b, anti-aliased)          absgrad 1.3e-7   signed 7.7e-7
      form d (aux_affine depth)         absgrad 1.8e-7   signed 5.9e-7
  — at most 7.7e-7, below a tenth of helpers.GRAD_RTOL (2e-6): the GPU comparison keeps `helpers.check_grads` as it stands.  The
  test below holds every form to that tenth."""
import numpy as np
import pytest
import torch

from oracle import torch_raster as tr
from tests import absgrad_reference as ar
from tests import contributions_reference as cr
from tests.helpers import GRAD_RTOL, rel_l2

W, H = ar.GPU_W, ar.GPU_H
_cache = {}


def _ref(form, dtype):
    if (form, dtype) not in _cache:
        _cache[(form, dtype)] = ar.form_reference(form, dtype)
    return _cache[(form, dtype)]


def test_the_scene_has_a_background_and_the_gradients_four_zero_columns():
    sc = ar.gpu_scene()
    assert float(sc.bg.abs().min()) > 0
    g = ar.upstream()
    for v in g.values():
        assert not bool(v[..., :4].any()) and bool(v[..., 4:].all())


@pytest.mark.parametrize("with_depth_alpha", [False, True], ids=["colour", "colour_depth_alpha"])
def test_signed_sums_are_the_oracles_autograd_gradient(with_depth_alpha):
    sc = ar.gpu_scene()
    g = {k: v.double() for k, v in ar.upstream().items()}
    c = lambda t: t.detach().double()
    pre, point_list, ranges = cr.lists(c(sc.means3D), c(sc.opacities), c(sc.viewmatrix), c(sc.projmatrix), c(sc.campos), W, H,
                                       sc.tanfovx, sc.tanfovy, sc.sh_degree, shs=c(sc.shs), cov3D_precomp=c(sc.cov3D), sh_cap=3)
    aux = c(ar.aux_value(sc))
    gD, gA = (g["gD"], g["gA"]) if with_depth_alpha else (None, None)
    absg, signed, planes = ar.absgrad_from_lists(pre, point_list, ranges, c(sc.bg), W, H, g["gC"], gD, gA, depth_value=aux)
    # the oracle: the same lists, autograd from the loss down to the 2D means
    p2 = dict(pre)
    p2["xy"] = pre["xy"].detach().clone().requires_grad_(True)
    color, _t, _n, depth = tr.blend(p2, point_list, ranges, c(sc.bg), W, H, aux=aux)
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    alpha = 1.0 - (tr.blend(p2, point_list, ranges, one, W, H, want_depth=False)[0][0] -
                   tr.blend(p2, point_list, ranges, zero, W, H, want_depth=False)[0][0])
    loss = (color * g["gC"]).sum()
    if with_depth_alpha:
        loss = loss + (depth * gD).sum() + (alpha * gA).sum()
    (dxy,) = torch.autograd.grad(loss, p2["xy"])
    want = dxy * torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64)
    assert torch.equal(planes["color"], color.detach()) and torch.equal(planes["depth"], depth.detach())
    assert float((planes["alpha"] - alpha.detach()).abs().max()) <= 1e-14
    r = rel_l2(signed.numpy(), want.numpy())
    print(f"signed vs oracle autograd: rel-L2 {r:.3e}, |want| {float(want.norm()):.3e}")
    assert float(want.norm()) > 0 and r <= 1e-10
    assert bool((absg >= signed.abs() * (1.0 - 1e-12)).all())


@pytest.mark.parametrize("form", list(ar.FORMS))
def test_absgrad_dominates_the_signed_sums_and_cancellation_is_common(form):
    absg, signed, _planes, count = _ref(form, torch.float64)
    assert bool((absg >= signed.abs() * (1.0 - 1e-12)).all())
    seen = count > 0
    assert int(seen.sum()) > 300 and not bool(absg[~seen].any()) and not bool(signed[~seen].any())
    share = float((absg[seen, 0] > 1.5 * signed[seen, 0].abs()).double().mean())
    print(f"{form}: {int(seen.sum())} composited Gaussians, absgrad_x > 1.5·|signed_x| for {share:.3f} of them")
    assert share >= 0.5


@pytest.mark.parametrize("form", list(ar.FORMS))
def test_float32_run_against_float64_run_is_the_rounding_floor(form):
    a64, s64, _p, _c = _ref(form, torch.float64)
    a32, s32, _p, _c = _ref(form, torch.float32)
    ra, rs = rel_l2(a32.numpy(), a64.numpy()), rel_l2(s32.numpy(), s64.numpy())
    print(f"{form}: float32 vs float64 rel-L2 absgrad {ra:.3e}, signed {rs:.3e}")
    assert np.isfinite(a32.numpy()).all() and np.isfinite(s32.numpy()).all()
    assert max(ra, rs) <= 0.1 * GRAD_RTOL
