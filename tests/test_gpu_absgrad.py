"""The absgrad pass on the GPU (`-m gpu`): the `absgrad` setting / ggr_means2d_absgrad.

The scene (tests/absgrad_reference.py `gpu_scene`): `distortion_reference.clustered_scene()` — a 40×24 frame, 3×2 tiles, ragged
right and bottom, of 700 Gaussians pulled towards tile (1, 0), whose list exceeds 512 entries (three LDS batches); pixels there
stop early, pixels near the edges run to the end of their lists — with a NON-ZERO background, so that the T_f·u_bg term is live.
The upstream gradients (`upstream()`) have four exactly-zero columns: those pixels take no entry.

Bar: helpers.check_grads as it stands — rel-L2 ≤ 1e-3 over all rows and ≤ GRAD_RTOL (2e-5) once the flip rule's rows are set
aside (none at 700 rows: the rule is proportional, so 2e-5 holds over all rows).  It is kept because the rounding floor —
the float64 reference against its own float32 run, tests/test_absgrad_reference.py — is at most 7.7e-7 on this scene, below a
tenth of GRAD_RTOL.  tests/test_absgrad_reference.py also asserts the condition without which a kernel returning the signed sums
would pass: absgrad_x > 1.5·|signed_x| for more than half of the composited Gaussians (77 … 79 % here).
Measured on an MI355X against the float64 reference, rel-L2 over all rows of the four forms: absgrad 1.7e-7 … 2.6e-7, the signed
sums 1.1e-6 … 3.7e-6 (means2D.grad of the same backward: 7.1e-7 … 9.0e-7).

"Bit-identical" is said of planes.  Gradients of two runs are compared within rounding: they are accumulated with float atomics
in varying order."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views
from tests import absgrad_reference as ar
from tests.helpers import GRAD_RTOL, check_grads, check_image, rel_l2
from tests.test_gpu_alpha import _cams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, P = ar.GPU_W, ar.GPU_H, ar.GPU_P
K = 4

_cache = {}


def _scene():
    if "scene" not in _cache:
        _cache["scene"] = ar.gpu_scene()
    return _cache["scene"]


def _reference(form):
    """float64 reference of one input form — computed once per process, read only"""
    if form not in _cache:
        absg, signed, planes, count = ar.form_reference(form, torch.float64, sc=_scene())
        _cache[form] = (absg.numpy(), signed.numpy(), {k: v.numpy() for k, v in planes.items()}, count.numpy())
    return _cache[form]


def _run(sc, g, form, absgrad=True, extra_loss=None, feats=None, **extra):
    """Forward + backward of one of ar.FORMS on cuda:0 under the upstream gradients `g` → dict(planes…, m2d = the means2D leaf,
    grads = the leaves' gradients).  `extra_loss(out) -> tensor` is added to the loss."""
    f = ar.FORMS[form]
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    means, op = leaf(s.means3D), leaf(s.opacities)
    kw, leaves = {}, dict(means3D=means, opacities=op)
    if f["use_sh"]:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(ar.colors())
    if f["use_cov"]:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(s.scales)
        leaves["rotations"] = kw["rotations"] = leaf(s.rotations)
    if f.get("aux"):
        leaves["aux"] = kw["aux_precomp"] = leaf(ar.aux_value(sc))
    if feats is not None:
        leaves["features"] = kw["features_precomp"] = leaf(feats)
    rs = s.settings()._replace(sh_max_degree=3, absgrad=absgrad, return_alpha=f["alpha"],
                               antialiasing=f.get("antialiasing", False), aux_affine=ar.AFFINE if f.get("affine") else None, **extra)
    m2d = torch.zeros_like(means, requires_grad=True)
    tup = GaussianRasterizer(rs)(means3D=means, means2D=m2d, opacities=op, **kw)
    names = ["color", "radii", "depth"] + (["alpha"] if f["alpha"] else []) + (["features"] if feats is not None else []) + \
        (["distortion"] if extra.get("return_distortion") else []) + (["contributions"] if extra.get("return_contributions") else [])
    assert len(tup) == len(names)
    out = dict(zip(names, tup))
    loss = (out["color"] * g["gC"].to(DEV)).sum()
    if f["depth"]:
        loss = loss + (out["depth"] * g["gD"].to(DEV)).sum()
    if f["alpha"]:
        loss = loss + (out["alpha"] * g["gA"].to(DEV)).sum()
    if extra_loss is not None:
        loss = loss + extra_loss(out)
    loss.backward()
    torch.cuda.synchronize()
    leaves["means2D"] = m2d
    out["grads"] = {k: v.grad.detach().cpu().numpy() for k, v in leaves.items() if v.grad is not None}
    out["m2d"] = m2d
    return out


def _attrs(m2d):
    a, s = m2d.absgrad, m2d.absgrad_signed
    assert a.dtype == torch.float32 and s.dtype == torch.float32 and not a.requires_grad and not s.requires_grad
    assert a.grad_fn is None and s.grad_fn is None and a.device == m2d.device
    return a.cpu().numpy(), s.cpu().numpy()


# ---- 1. against the float64 reference ---------------------------------------------------------------------------------------------
def test_the_scene_has_a_background_and_a_long_list():
    import ggrt_official_amd.rasterizer as R
    sc = _scene()
    assert float(sc.bg.abs().min()) > 0
    _run(sc, ar.upstream(), "a_sh_cov_colour_only")
    assert R.last_forward_binning()[1] > 512, "no tile list of three LDS batches"


@pytest.mark.parametrize("form", list(ar.FORMS))
def test_absgrad_and_signed_sums_match_the_float64_reference(form):
    ref_abs, ref_signed, planes, count = _reference(form)
    out = _run(_scene(), ar.upstream(), form, return_contributions=True)
    a, s = _attrs(out["m2d"])
    assert a.shape == (P, 2) and s.shape == (P, 2)
    assert np.isfinite(a).all() and np.isfinite(s).all() and (a >= 0).all()
    # (the reference's planes are the product's: the comparison below is about the pass, not about another frame)
    check_image(out["color"].detach().cpu().numpy(), planes["color"], name="color", tag=f"absgrad:color:{form}")
    m2 = out["grads"]["means2D"][:, :2]
    print(f"{form}: rel-L2 absgrad {rel_l2(a, ref_abs):.3e}, signed {rel_l2(s, ref_signed):.3e}, "
          f"signed vs means2D.grad {rel_l2(s, m2):.3e}, means2D.grad vs reference {rel_l2(m2, ref_signed):.3e}; "
          f"|absgrad| {np.linalg.norm(ref_abs):.3e}, |signed| {np.linalg.norm(ref_signed):.3e}")
    assert np.linalg.norm(ref_abs) > 2.0 * np.linalg.norm(ref_signed) > 0
    check_grads(dict(absgrad=a, absgrad_signed=s), dict(absgrad=ref_abs, absgrad_signed=ref_signed),
                ["absgrad", "absgrad_signed"], tag=f"absgrad:{form}")
    check_grads(dict(absgrad_signed=s), dict(absgrad_signed=m2), ["absgrad_signed"], tag=f"absgrad:m2d:{form}")
    assert (a >= np.abs(s) * (1.0 - 1e-4)).all()
    # never composited (the product's own count): exactly zero
    pc = out["contributions"].pixel_count.cpu().numpy()
    assert abs(int((pc > 0).sum()) - int((count > 0).sum())) <= 2
    assert (pc == 0).sum() > 100 and not a[pc == 0].any() and not s[pc == 0].any()


# ---- 2. on / off ------------------------------------------------------------------------------------------------------------------
def test_off_is_the_parent_and_on_changes_no_plane(monkeypatch):
    lib = _lib.load()
    sc, g, form = _scene(), ar.upstream(), "b_colours_scale_rot_aux_depth_alpha"
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_means2d_absgrad", lambda *a: calls.append("a") or 99)
        off = _run(sc, g, form, absgrad=False)
    assert not calls and not hasattr(off["m2d"], "absgrad") and not hasattr(off["m2d"], "absgrad_signed")
    on = _run(sc, g, form)
    assert hasattr(on["m2d"], "absgrad")
    for k in ("color", "radii", "depth", "alpha"):
        assert torch.equal(off[k], on[k]), k
    assert set(on["grads"]) == set(off["grads"])
    for k in off["grads"]:
        assert np.abs(off["grads"][k]).max() > 0 and rel_l2(on["grads"][k], off["grads"][k]) <= GRAD_RTOL, k


def test_nothing_runs_without_a_backward(monkeypatch):
    lib = _lib.load()
    s = _scene().to(DEV)
    calls = []
    monkeypatch.setattr(lib, "ggr_means2d_absgrad", lambda *a: calls.append("a") or 99)
    rs = s.settings()._replace(sh_max_degree=3, absgrad=True)
    m2d = torch.zeros_like(s.means3D, requires_grad=True)
    with torch.no_grad():
        GaussianRasterizer(rs)(means3D=s.means3D, means2D=m2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)
    m2 = torch.zeros_like(s.means3D)
    GaussianRasterizer(rs)(means3D=s.means3D, means2D=m2, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)   # nothing requires grad
    torch.cuda.synchronize()
    assert not calls and not hasattr(m2d, "absgrad") and not hasattr(m2, "absgrad")


# ---- 3. what absgrad covers ---------------------------------------------------------------------------------------------------------
def test_feature_and_distortion_losses_change_the_gradient_but_not_absgrad():
    sc, g, form = _scene(), ar.upstream(), "b_colours_scale_rot_aux_depth_alpha"
    gen = torch.Generator().manual_seed(1411)
    feats = torch.rand(P, K, generator=gen) * 2.0 - 0.5
    gF = (torch.randn(K, H, W, generator=gen) / (3.0 * H * W)).to(DEV)
    gQ = (torch.randn(H, W, generator=gen) / (H * W)).to(DEV)
    base = _run(sc, g, form, feats=feats, return_distortion=True)
    more = _run(sc, g, form, feats=feats, return_distortion=True,
                extra_loss=lambda out: (out["features"] * gF).sum() + (out["distortion"] * gQ).sum())
    a0, s0 = _attrs(base["m2d"])
    a1, s1 = _attrs(more["m2d"])
    assert rel_l2(more["grads"]["means2D"], base["grads"]["means2D"]) > 1e-2      # the two losses reach means2D.grad …
    assert rel_l2(a1, a0) <= GRAD_RTOL and rel_l2(s1, s0) <= GRAD_RTOL             # … and are not part of absgrad
    assert rel_l2(a0, _reference(form)[0]) <= GRAD_RTOL


# ---- 4. launch sets -----------------------------------------------------------------------------------------------------------------
def _per_view(s, rs, view, proj, cam, bg, gC):
    outs = []
    for v in range(view.shape[0]):
        m2 = torch.zeros_like(s.means3D, requires_grad=True)
        r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=bg[v], tanfovx=s.tanfovx, tanfovy=s.tanfovy)
        c = GaussianRasterizer(r)(means3D=s.means3D.clone().requires_grad_(True), means2D=m2, opacities=s.opacities, shs=s.shs,
                                  cov3D_precomp=s.cov3D)[0]
        (c * gC[v]).sum().backward()
        outs.append((m2.absgrad, m2.absgrad_signed))
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def test_launch_set_and_gaussian_sets_equal_per_view_calls():
    scs = [ar.gpu_scene(seed=ar.GPU_SEED + b).to(DEV) for b in range(2)]
    scs[1].bg = torch.tensor([0.7, 0.2, 0.4], device=DEV)
    gC = torch.stack([ar.upstream(1420 + v)["gC"] for v in range(4)]).to(DEV)
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 4, dtype=torch.float32, device=DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3, absgrad=True)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    # one Gaussian set, two views
    s = scs[0]
    view, proj, cam = _cams(s, 2)
    bg = s.bg.reshape(1, 3).expand(2, 3).contiguous()
    m2 = torch.zeros(2, P, 3, device=DEV, requires_grad=True)
    out = rasterize_views(leaf(s.means3D), s.opacities, view, proj, cam, bg, tf[:2], rs, shs=s.shs, cov3D_precomp=s.cov3D, means2D=m2)
    (out[0] * gC[:2]).sum().backward()
    assert m2.absgrad.shape == (2, P, 2) and m2.absgrad_signed.shape == (2, P, 2) and m2.absgrad.dtype == torch.float32
    ref_a, ref_s = _per_view(s, rs, view, proj, cam, bg, gC[:2])
    for v in range(2):
        assert float(ref_a[v].max()) > 0
        assert rel_l2(m2.absgrad[v].cpu().numpy(), ref_a[v].cpu().numpy()) <= GRAD_RTOL
        assert rel_l2(m2.absgrad_signed[v].cpu().numpy(), ref_s[v].cpu().numpy()) <= GRAD_RTOL
    assert rel_l2(m2.absgrad_signed.cpu().numpy(), m2.grad[..., :2].cpu().numpy()) <= GRAD_RTOL
    with pytest.raises(ValueError, match="means2D"):
        rasterize_views(leaf(s.means3D), s.opacities, view, proj, cam, bg, tf[:2], rs, shs=s.shs, cov3D_precomp=s.cov3D)
    # four views over two Gaussian sets: rows are per (view, Gaussian of that view's set)
    cams = [_cams(s_, 2) for s_ in scs]
    view, proj, cam = (torch.cat([c_[i] for c_ in cams]) for i in range(3))
    bg = torch.stack([scs[v // 2].bg for v in range(4)])
    stk = lambda f: torch.stack([f(s_) for s_ in scs])
    m2 = torch.zeros(4, P, 3, device=DEV, requires_grad=True)
    out = rasterize_views(leaf(stk(lambda s_: s_.means3D)), stk(lambda s_: s_.opacities), view, proj, cam, bg, tf, rs,
                          shs=stk(lambda s_: s_.shs), cov3D_precomp=stk(lambda s_: s_.cov3D), means2D=m2)
    (out[0] * gC).sum().backward()
    assert m2.absgrad.shape == (4, P, 2)
    for b in range(2):
        ref_a, ref_s = _per_view(scs[b], rs, *cams[b], bg[2 * b:2 * b + 2], gC[2 * b:2 * b + 2])
        for v in range(2):
            assert rel_l2(m2.absgrad[2 * b + v].cpu().numpy(), ref_a[v].cpu().numpy()) <= GRAD_RTOL, (b, v)
            assert rel_l2(m2.absgrad_signed[2 * b + v].cpu().numpy(), ref_s[v].cpu().numpy()) <= GRAD_RTOL, (b, v)


# ---- 5. modes -----------------------------------------------------------------------------------------------------------------------
def test_a_scissored_frame_equals_the_full_frame_under_a_gradient_confined_to_the_tile():
    sc, form = _scene(), "b_colours_scale_rot_aux_depth_alpha"
    g = {k: v.clone() for k, v in ar.upstream().items()}
    mask = torch.zeros(H, W, dtype=torch.bool)
    mask[0:16, 16:32] = True
    for v in g.values():
        v[..., ~mask] = 0.0
    full = _run(sc, g, form)
    win = _run(sc, g, form, scissor=(16, 0, 32, 16))
    a0, s0 = _attrs(full["m2d"])
    a1, s1 = _attrs(win["m2d"])
    assert np.abs(a0).max() > 0 and rel_l2(a1, a0) <= GRAD_RTOL and rel_l2(s1, s0) <= GRAD_RTOL
    assert np.array_equal(a0 == 0, a1 == 0)


def test_sync_free_mode_equals_exact_mode():
    sc, g, form = _scene(), ar.upstream(), "b_colours_scale_rot_aux_depth_alpha"
    a0, s0 = _attrs(_run(sc, g, form)["m2d"])
    a1, s1 = _attrs(_run(sc, g, form, list_capacity=20_000)["m2d"])
    assert rel_l2(a1, a0) <= GRAD_RTOL and rel_l2(s1, s0) <= GRAD_RTOL
    assert rel_l2(a1, _reference(form)[0]) <= GRAD_RTOL


def test_a_second_backward_overwrites_the_attribute():
    s = _scene().to(DEV)
    g1, g2 = ar.upstream()["gC"].to(DEV), 3.0 * ar.upstream(1430)["gC"].to(DEV)   # (another pattern at three times the size)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    m, m2d = leaf(s.means3D), torch.zeros_like(s.means3D, requires_grad=True)
    rs = s.settings()._replace(sh_max_degree=3, absgrad=True)
    color = GaussianRasterizer(rs)(means3D=m, means2D=m2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)[0]
    color.backward(g1, retain_graph=True)
    first = m2d.absgrad.clone()
    color.backward(g2)
    second = m2d.absgrad.clone()
    # each equals a fresh forward + backward under its own gradient
    for grad, got in ((g1, first), (g2, second)):
        f2d = torch.zeros_like(s.means3D, requires_grad=True)
        c = GaussianRasterizer(rs)(means3D=leaf(s.means3D), means2D=f2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)[0]
        c.backward(grad)
        assert float(f2d.absgrad.max()) > 0 and rel_l2(got.cpu().numpy(), f2d.absgrad.cpu().numpy()) <= GRAD_RTOL
    assert rel_l2(second.cpu().numpy(), first.cpu().numpy()) > 1.0     # overwritten, and neither kept nor accumulated


def test_empty_frames_give_zeros_of_the_right_shape():
    s = _scene().to(DEV)
    rs = s.settings()._replace(sh_max_degree=3, absgrad=True)
    z = lambda *sh: torch.zeros(*sh, device=DEV, requires_grad=True)
    m2d = z(0, 3)
    color = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=m2d, opacities=z(0, 1), shs=z(0, 4, 3), cov3D_precomp=z(0, 6))[0]
    color.sum().backward()
    assert m2d.absgrad.shape == (0, 2) and m2d.absgrad_signed.shape == (0, 2)
    # everything behind the camera: num_rendered = 0
    m = s.means3D.clone()
    m[:, 2] = -m[:, 2]
    m.requires_grad_(True)
    m2d = torch.zeros_like(m, requires_grad=True)
    color = GaussianRasterizer(rs)(means3D=m, means2D=m2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)[0]
    (color * ar.upstream()["gC"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert m2d.absgrad.shape == (P, 2) and not bool(m2d.absgrad.any()) and not bool(m2d.absgrad_signed.any())
