"""The projection pass on the GPU (`-m gpu`): `return_projection` / ggr_projection / ggr_projection_backward.

With `return_projection=True` a call returns, last, a `Projection(means2d, depth, conic, opacity, color, valid)` of per-Gaussian
rows: the geometry buffer's own bits on valid rows, 0 elsewhere, the five float fields differentiable.  Checked: the values against
`ggr_debug_unpack_geom` bit for bit, the gradients against the float64 torch reference (tests/projection_reference.py: the frozen
oracle's `preprocess` + autograd), NaN on invalid rows, composition with the image / feature / hit-weight losses in one scratch,
launch sets, the edges (P = 0, 1, an all-invalid frame, the scissor, a second backward, no_grad, graph capture) and "off = as
before".

Scenes: hits_reference.REF_CASES with eight invalid rows appended to each (tests/projection_reference.py), P + 8 = 6008 / 6008 /
1008 rows — none a multiple of 64.  tests/test_projection_reference.py fixes on the CPU that the float32 and float64 references
agree on `valid`, so the GPU is held to equality there before any gradient is compared.

The repo's conic convention (stated here because test 1 maps `conic_opacity` by it): `conic = (a, b, c)` with
power = −½(a·dx² + c·dy²) − b·dx·dy, the inverse of the dilated 2D covariance — `ggr_debug_unpack_geom`'s `conic_opacity` row is
(a, b, c, opacity), `oracle.torch_raster.preprocess`' `conic` is (a, b, c).

Bars.  Gradients against the reference: helpers.check_grads unchanged (rel-L2 ≤ 1e-3 over all rows, ≤ GRAD_RTOL = 2e-5 once the
flip rule's rows are set aside — none at these sizes), the camera tensors and tanfov at GRAD_RTOL_ALL like the existing
camera-gradient tests.  Two HIP runs that sum the same terms are compared within GRAD_RTOL (the blend backward's float atomics),
the camera tensors and tanfov of a launch set against the per-view calls included."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, PixelHits, Projection, _lib, rasterize_views
from ggrt_official_amd.rasterizer import debug_forward_state
from ggrt_official_amd.synthetic import make_scene, upstream_gradient
from tests import projection_reference as pj
from tests.helpers import GRAD_RTOL, GRAD_RTOL_ALL, check_grads, rel_l2
from tests.test_gpu_alpha import _cams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(pj.REF_CASES)
A, B, Cs = NAMES   # A_sh_cov, B_colours_scale_rot_aa_odd_frame, C_small_gaussians_unfilled_slots
FIELDS = list(pj.FIELDS)
CAMS = ["viewmatrix", "projmatrix", "campos", "tanfov"]


def _inputs(name):
    """input names of a reference scene, in its own form: geometry + colour"""
    _P, _W, _H, _D, use_sh, use_cov, _aa, _seed = pj.REF_CASES[name]
    return (["means3D", "opacities"] + (["cov3D_precomp"] if use_cov else ["scales", "rotations"])
            + (["shs"] if use_sh else ["colors_precomp"]))


def _g(name, seed=2201):
    """fixed upstream gradients of mixed sign, one per differentiable field (CPU, float32)"""
    shapes = pj.ref_projection(name)
    gen = torch.Generator().manual_seed(seed)
    return {f: torch.randn(shapes[f].shape, generator=gen) for f in FIELDS}


def _leaves(name, pose=False):
    """(scene on the device, rasterizer keyword inputs, leaves by name) of a reference scene in its own input form"""
    sc, colors = pj.ref_scene(name)
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    src = dict(means3D=s.means3D, opacities=s.opacities, cov3D_precomp=s.cov3D, scales=s.scales, rotations=s.rotations,
               shs=s.shs, colors_precomp=colors)
    leaves = {k: leaf(src[k]) for k in _inputs(name)}
    kw = dict(leaves)
    if pose:
        leaves.update(viewmatrix=leaf(s.viewmatrix), projmatrix=leaf(s.projmatrix), campos=leaf(s.campos),
                      tanfov=leaf(torch.tensor([s.tanfovx, s.tanfovy], dtype=torch.float32)))
    return s, kw, leaves


def _settings(name, s, leaves, **settings):
    settings.setdefault("antialiasing", pj.REF_CASES[name][6])
    settings.setdefault("return_projection", True)
    rs = s.settings()._replace(sh_max_degree=3, **settings)
    if "viewmatrix" in leaves:
        rs = rs._replace(viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"], campos=leaves["campos"],
                         tanfov=leaves["tanfov"])
    return rs


def _forward(name, pose=False, features=None, aux=None, **settings):
    s, kw, leaves = _leaves(name, pose)
    rs = _settings(name, s, leaves, **settings)
    if features is not None:
        leaves["features"] = kw["features_precomp"] = features.detach().clone().to(DEV).requires_grad_(True)
    if aux is not None:
        leaves["aux"] = kw["aux_precomp"] = aux.detach().clone().to(DEV).requires_grad_(True)
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    out = GaussianRasterizer(rs)(means2D=leaves["means2D"], **kw)
    assert not rs.return_projection or isinstance(out[-1], Projection)
    return out, leaves


def _proj_loss(p, g):
    return sum((getattr(p, f) * t.to(DEV)).sum() for f, t in g.items())


def _np_grads(leaves):
    torch.cuda.synchronize()
    return {k: (np.zeros(tuple(v.shape), np.float32) if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}


def _run(name, g, pose=False, more=None, **kw):
    """forward + backward of Σ_f Σ g[f]·field_f (`more(out)` adds to the loss) → (out, grads)"""
    out, leaves = _forward(name, pose, **kw)
    loss = _proj_loss(out[-1], g) if g else 0.0
    if more is not None:
        loss = loss + more(out)
    loss.backward()
    return out, _np_grads(leaves)


def _close(a, b, keys, tag, rtol=GRAD_RTOL):
    for k in keys:
        r = rel_l2(a[k], b[k])
        print(f"{tag} {k}: rel-L2 {r:.3e}, |ref| {np.linalg.norm(b[k]):.3e}")
        assert np.isfinite(a[k]).all() and np.linalg.norm(b[k]) > 0 and r <= rtol, (tag, k, r)


# ---- 1. forward values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fields_are_the_geometry_buffers_bits(name):
    P = pj.REF_CASES[name][0] + pj.N_EXTRA
    with torch.no_grad():
        out, leaves = _forward(name)
    p, radii = out[-1], out[1]
    assert len(out) == 4 and [tuple(t.shape) for t in p] == [(P, 2), (P,), (P, 3), (P,), (P, 3), (P,)]
    assert all(t.dtype == torch.float32 for t in p[:5]) and p.valid.dtype == torch.bool
    s, kw, _ = _leaves(name)
    st = debug_forward_state(raster_settings=_settings(name, s, {}, return_projection=False),
                             **{k: v.detach() for k, v in kw.items()})
    v = p.valid
    assert torch.equal(v, radii > 0) and torch.equal(radii, st["radii"])
    ref = pj.ref_projection(name, torch.float32)
    assert torch.equal(v.cpu(), ref["valid"]), "valid differs from the reference's"
    assert int((~v).sum()) >= 8 and int(v.sum()) >= 8
    co = st["conic_opacity"]   # rows (a, b, c, opacity): the conic convention of this file's docstring
    want = dict(means2d=st["xy"], depth=st["depth"], conic=co[:, :3], opacity=co[:, 3], color=st["rgb"])
    for f in FIELDS:
        got = getattr(p, f)
        assert torch.equal(got[v], want[f][v]), f                  # bit for bit on valid rows
        assert not bool(got[~v].any()) and not bool(torch.signbit(got[~v]).any()), f   # exactly +0 on the others
        assert torch.allclose(got.cpu(), ref[f], rtol=1e-3, atol=1e-3), f   # (and the oracle's values, loosely: test_gpu_parity pins them)


@pytest.mark.parametrize("name", [A, B])
def test_depth_is_the_aux_value_when_aux_is_given(name):
    P = pj.REF_CASES[name][0] + pj.N_EXTRA
    aux = torch.randn(P, generator=torch.Generator().manual_seed(2202))
    with torch.no_grad():
        out, _l = _forward(name, aux=aux)
        plain, _l = _forward(name)
    p = out[-1]
    assert torch.equal(p.depth[p.valid], aux.to(DEV)[p.valid]) and not bool(p.depth[~p.valid].any())
    for f in ("means2d", "conic", "opacity", "color", "valid"):
        assert torch.equal(getattr(p, f), getattr(plain[-1], f)), f


# ---- 2. gradients against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", FIELDS + ["all"])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_the_float64_reference(name, which):
    g = _g(name)
    g = g if which == "all" else {which: g[which]}
    out, grads = _run(name, g, pose=True)
    p = out[-1]
    assert all(getattr(p, f).requires_grad for f in FIELDS) and not p.valid.requires_grad
    assert torch.equal(p.valid.cpu(), pj.ref_projection(name)["valid"])
    want = pj.ref_grads(name, g)
    keys = _inputs(name)
    for k in keys + CAMS:
        print(f"{name} {which} grad {k}: rel-L2 {rel_l2(grads[k], want[k]):.3e}, |ref| {np.linalg.norm(want[k]):.3e}, "
              f"|got| {np.linalg.norm(grads[k]):.3e}")
    assert any(np.linalg.norm(want[k]) > 0 for k in keys)
    invalid = ~p.valid.cpu().numpy()
    for k in keys:   # an invalid row gets nothing, in any input
        assert not np.any(grads[k][invalid]), k
    check_grads(grads, want, keys, tag=f"projection:{name}:{which}")
    for k in CAMS:   # (the bar of the existing camera-gradient tests; a tensor the loss does not reach is exactly zero)
        if np.linalg.norm(want[k]) > 0:
            assert rel_l2(grads[k], want[k]) <= GRAD_RTOL_ALL, k
        else:
            assert not np.any(grads[k]), k
    # the means2D sink: the means2d term in the sink's own (NDC) units — pixel = ((ndc + 1)·W − 1)/2
    sink = grads["means2D"]
    if "means2d" in g:
        W, H = pj.REF_CASES[name][1:3]
        gm = np.where(invalid[:, None], 0.0, g["means2d"].numpy()) * np.array([0.5 * W, 0.5 * H], np.float32)
        assert np.allclose(sink[:, :2], gm, rtol=1e-6, atol=0) and not np.any(sink[:, 2])
    else:
        assert not np.any(sink)


def test_depth_gradient_reaches_aux_when_aux_is_given():
    name = A
    P = pj.REF_CASES[name][0] + pj.N_EXTRA
    aux = torch.randn(P, generator=torch.Generator().manual_seed(2203))
    g = {"depth": _g(name)["depth"]}
    out, grads = _run(name, g, aux=aux)
    want = pj.ref_grads(name, g, aux=aux)
    valid = out[-1].valid.cpu().numpy()
    assert np.array_equal(grads["aux"], np.where(valid, g["depth"].numpy(), 0.0)) and np.array_equal(grads["aux"], want["aux"].astype(np.float32))
    assert not np.any(grads["means3D"]) and not np.any(want["means3D"])   # the depth value no longer depends on the geometry


# ---- 3. invalid rows are ignored ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_nan_on_invalid_rows_reaches_no_result(name):
    g = _g(name)
    invalid = ~pj.ref_projection(name)["valid"]
    nan = {f: torch.where(invalid if t.dim() == 1 else invalid[:, None], torch.full((), float("nan")), t) for f, t in g.items()}
    zero = {f: torch.where(invalid if t.dim() == 1 else invalid[:, None], torch.zeros(()), t) for f, t in g.items()}
    assert all(bool(torch.isnan(t[invalid]).all()) for t in nan.values())
    res = {}   # (the gradients are handed in directly: a product with a NaN would be NaN before it reached the rasterizer)
    for tag, grads_in in (("nan", nan), ("zero", zero)):
        out, leaves = _forward(name, pose=True)
        torch.autograd.backward([getattr(out[-1], f) for f in FIELDS], [grads_in[f].to(DEV) for f in FIELDS])
        res[tag] = _np_grads(leaves)
    keys = _inputs(name) + CAMS + ["means2D"]
    for k in keys:
        assert np.isfinite(res["nan"][k]).all(), k
    # (campos is reached through the SH view direction only: with colors_precomp its gradient is exactly zero in both runs)
    _P, _W, _H, _D, use_sh, _cov, _aa, _seed = pj.REF_CASES[name]
    if not use_sh:
        assert not np.any(res["nan"]["campos"]) and not np.any(res["zero"]["campos"])
        keys.remove("campos")
    _close(res["nan"], res["zero"], keys, f"nan on invalid rows {name}")


# ---- 4. composition ----------------------------------------------------------------------------------------------------------------
def test_image_projection_features_and_hits_in_one_backward_equal_four_backwards():
    name, K, KF = A, 4, 2
    P, W, H = pj.REF_CASES[name][0] + pj.N_EXTRA, *pj.REF_CASES[name][1:3]
    gen = torch.Generator().manual_seed(2211)
    g = {f: t / P for f, t in _g(name).items()}
    feats = torch.rand(P, KF, generator=gen) * 2.0 - 0.5
    gF = (torch.randn(KF, H, W, generator=gen) / (H * W)).to(DEV)
    gW, gR = (torch.randn(K, H, W, generator=gen) / (H * W)).to(DEV), (torch.randn(H, W, generator=gen) / (H * W)).to(DEV)
    dL = upstream_gradient(W, H, seed=2212).to(DEV)
    kw = dict(features=feats, return_hits=K, hits_grad=True)   # the tuple: colour, radii, depth, features, hits, projection
    img = lambda o: (o[0] * dL).sum()
    fea = lambda o: (o[3] * gF).sum()
    hit = lambda o: (o[4].weight * gW).sum() + (o[4].rest * gR).sum()
    out, all4 = _run(name, g, more=lambda o: img(o) + fea(o) + hit(o), **kw)
    assert isinstance(out[4], PixelHits) and isinstance(out[5], Projection) and len(out) == 6
    parts = [_run(name, {}, more=img, **kw)[1], _run(name, g, **kw)[1], _run(name, {}, more=fea, **kw)[1], _run(name, {}, more=hit, **kw)[1]]
    keys = _inputs(name) + ["features", "means2D"]
    want = {k: sum(p[k] for p in parts) for k in keys}
    assert all(np.abs(p[k]).max() > 0 for p in parts for k in _inputs(name)[:3])
    _close(all4, want, keys, "image + projection + features + hits")
    # … and the projection loss with each of the others alone (it is seeded last, behind whoever cleared the scratch)
    for tag, fn, i in (("features", fea, 2), ("hits", hit, 3)):
        _o, two = _run(name, g, more=fn, **kw)
        _close(two, {k: parts[1][k] + parts[i][k] for k in keys}, _inputs(name)[:3], f"projection + {tag}")


@pytest.mark.parametrize("only", FIELDS)
def test_a_loss_on_one_field_sends_null_for_the_other_four(only, monkeypatch):
    """… and no colour gradient at all (grad_color = None): the result equals the run with explicit zeros everywhere else"""
    name = Cs
    g = _g(name)
    lib = _lib.load()
    real, seen = lib.ggr_projection_backward, []

    def spy(st, vw, pp, stream):
        p = pp._obj
        seen.append(tuple(bool(getattr(p, "dL_d" + f)) for f in FIELDS) + (int(p.scratch_zeroed),))
        return real(st, vw, pp, stream)

    monkeypatch.setattr(lib, "ggr_projection_backward", spy)
    _o, missing = _run(name, {only: g[only]})
    assert seen == [tuple(f == only for f in FIELDS) + (1,)], "None must travel as NULL; the forward's scratch is clear"
    W, H = pj.REF_CASES[name][1:3]
    _o, zeros = _run(name, {f: (t if f == only else torch.zeros_like(t)) for f, t in g.items()},
                     more=lambda o: (o[0] * torch.zeros(3, H, W, device=DEV)).sum())
    assert seen[-1] == (True,) * 5 + (1,)
    keys = [k for k in _inputs(name) + ["means2D"] if np.any(zeros[k])]
    assert keys
    _close(missing, zeros, keys, f"only {only}")
    # a loss that touches no projection field makes no call
    n = len(seen)
    _run(name, {}, more=lambda o: o[0].sum())
    assert len(seen) == n


# ---- 5. launch sets ----------------------------------------------------------------------------------------------------------------
def _views_case(sets):
    """2 views of one Gaussian set (sets = 1) or 2 sets of 2 views (sets = 2): fields equal the single-view calls' bit for bit,
    gradients equal their sums"""
    P, W, H = 800, 83, 45
    scs = []
    for b in range(sets):
        sc = make_scene(P, W, H, sh_degree=1, seed=2221 + b)
        sc.cov3D = sc.cov3D * 0.05
        sc.means3D[-4:, 2] = 0.1     # four behind the near cull …
        sc.means3D[-8:-4, 0] = 500.0   # … and four far outside the frustum
        scs.append(sc.to(DEV))
    V = 2 * sets
    gen = torch.Generator().manual_seed(2223)
    g = {f: torch.randn((V, P) + tuple(t.shape[1:]), generator=gen).to(DEV) for f, t in _g(Cs).items()}
    rs = scs[0].settings()._replace(sh_max_degree=3, return_projection=True)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    tf = leaf(torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * V, dtype=torch.float32, device=DEV))
    cams = [_cams(s, 2) for s in scs]
    view, proj, cam = (leaf(torch.cat([c[i] for c in cams])) for i in range(3))
    bg = torch.stack([s.bg for s in scs for _ in range(2)])
    stk = (lambda f: leaf(torch.stack([f(s) for s in scs]))) if sets > 1 else (lambda f: leaf(f(scs[0])))
    m, o, c, sh = stk(lambda s: s.means3D), stk(lambda s: s.opacities), stk(lambda s: s.cov3D), stk(lambda s: s.shs)
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=sh, cov3D_precomp=c)
    p = out[-1]
    assert isinstance(p, Projection) and p.means2d.shape == (V, P, 2) and p.valid.shape == (V, P) and p.color.shape == (V, P, 3)
    assert all(getattr(p, f).requires_grad for f in FIELDS) and not p.valid.requires_grad
    assert int((~p.valid).sum()) >= 8 * V and int(p.valid.sum()) >= 8 * V
    sum((getattr(p, f) * g[f]).sum() for f in FIELDS).backward()
    assert m.grad.shape == m.shape
    per_view = {k: [] for k in ("view", "proj", "cam", "tanfov")}
    for b, s in enumerate(scs):
        mb, ob, cb, sb = leaf(s.means3D), leaf(s.opacities), leaf(s.cov3D), leaf(s.shs)
        for v in range(2):
            n = 2 * b + v
            vv, pv, cv, tv = leaf(view[n]), leaf(proj[n]), leaf(cam[n]), leaf(tf[n])
            r = rs._replace(viewmatrix=vv, projmatrix=pv, campos=cv, bg=s.bg, tanfov=tv)
            pn = GaussianRasterizer(r)(means3D=mb, means2D=torch.zeros_like(mb), opacities=ob, shs=sb, cov3D_precomp=cb)[-1]
            for f in Projection._fields:
                assert torch.equal(getattr(pn, f).detach(), getattr(p, f)[n].detach()), (n, f)
            sum((getattr(pn, f) * g[f][n]).sum() for f in FIELDS).backward()
            for k, t in (("view", vv), ("proj", pv), ("cam", cv), ("tanfov", tv)):
                per_view[k].append(t.grad)
        pick = (lambda t: t.grad[b]) if sets > 1 else (lambda t: t.grad)
        for tag, a, r_ in zip(("means3D", "opacities", "cov3D", "shs"), (pick(m), pick(o), pick(c), pick(sh)),
                              (mb.grad, ob.grad, cb.grad, sb.grad)):
            rr = rel_l2(a.cpu().numpy(), r_.cpu().numpy())
            print(f"sets={sets} set {b} {tag}: rel-L2 {rr:.3e}")
            assert float(r_.abs().max()) > 0 and rr <= GRAD_RTOL, tag
    # the camera tensors and tanfov: both sides are HIP runs of the same projection-only loss, so they are held to GRAD_RTOL too
    for k, t in (("view", view), ("proj", proj), ("cam", cam), ("tanfov", tf)):
        want = torch.stack(per_view[k]).cpu().numpy()
        rr = rel_l2(t.grad.cpu().numpy(), want)
        print(f"sets={sets} {k}: rel-L2 {rr:.3e}, |ref| {np.linalg.norm(want):.3e}")
        assert t.grad.shape == t.shape and np.linalg.norm(want) > 0 and rr <= GRAD_RTOL, k


def test_two_views_of_one_set_equal_per_view_calls():
    _views_case(1)


def test_two_views_of_two_gaussian_sets_equal_per_view_calls():
    _views_case(2)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------
def _tiny(P, behind=False, seed=2231, **settings):
    sc = make_scene(max(P, 1), 40, 24, sh_degree=1, seed=seed)
    s = sc.to(DEV)
    leaf = lambda t: t[:P].detach().clone().requires_grad_(True)
    m = leaf(s.means3D)
    if behind:
        with torch.no_grad():
            m[:, 2] = -m[:, 2]
    leaves = dict(means3D=m, opacities=leaf(s.opacities), shs=leaf(s.shs), cov3D_precomp=leaf(s.cov3D))
    rs = s.settings()._replace(sh_max_degree=3, return_projection=True, **settings)
    out = GaussianRasterizer(rs)(means2D=torch.zeros_like(m, requires_grad=True), **leaves)
    return out, leaves


@pytest.mark.parametrize("P", [0, 1, 300])
def test_small_and_odd_sizes(P):
    out, leaves = _tiny(P)
    p = out[-1]
    assert [tuple(t.shape) for t in p] == [(P, 2), (P,), (P, 3), (P,), (P, 3), (P,)]
    assert torch.equal(p.valid, out[1] > 0)
    sum(getattr(p, f).sum() for f in FIELDS).backward()
    torch.cuda.synchronize()
    for k, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()), k
    if P:
        assert bool(p.valid.any()) and float(leaves["means3D"].grad.abs().max()) > 0
        assert bool((leaves["opacities"].grad.reshape(-1) == p.valid.float()).all())   # d(Σ opacity)/d opacity = 1 on valid rows


def test_a_frame_where_every_gaussian_is_invalid():
    out, leaves = _tiny(300, behind=True)
    p = out[-1]
    assert not bool(p.valid.any()) and not bool((out[1] > 0).any())
    for f in FIELDS:
        assert not bool(getattr(p, f).any()), f
    nan = lambda t: torch.full_like(t, float("nan"))
    torch.autograd.backward([getattr(p, f) for f in FIELDS], [nan(getattr(p, f)) for f in FIELDS])
    torch.cuda.synchronize()
    for k, t in leaves.items():
        assert t.grad is not None and not bool(t.grad.any()), k


def test_fields_do_not_depend_on_the_scissor():
    """`valid` is `radii > 0`, and the radii of a scissored forward refer to the window (a Gaussian that touches no window tile
    has radius 0): rows valid under the scissor hold the full frame's bits, the others 0 — nothing else changes"""
    name = A
    with torch.no_grad():
        full, _l = _forward(name)
        win, _l = _forward(name, scissor=(32, 16, 64, 48))
    pf, pw = full[-1], win[-1]
    assert torch.equal(pw.valid, win[1] > 0) and bool((pf.valid | ~pw.valid).all()) and 8 <= int(pw.valid.sum()) < int(pf.valid.sum())
    for f in FIELDS:
        a, b = getattr(pw, f), getattr(pf, f)
        assert torch.equal(a[pw.valid], b[pw.valid]) and not bool(a[~pw.valid].any()), f


def test_a_second_backward_over_one_forward():
    name = Cs
    g = _g(name)
    out, leaves = _forward(name)
    loss = _proj_loss(out[-1], g)
    ins = [leaves[k] for k in _inputs(name)]
    g1 = torch.autograd.grad(loss, ins, retain_graph=True)
    g2 = torch.autograd.grad(loss, ins)   # (a scratch of its own, not yet clear: the seeding pass clears it)
    for k, a, b in zip(_inputs(name), g1, g2):
        r = rel_l2(b.cpu().numpy(), a.cpu().numpy())
        print(f"second backward {k}: rel-L2 {r:.3e}")
        assert float(a.abs().max()) > 0 and r <= GRAD_RTOL, k


def test_no_grad_gives_detached_fields_and_keeps_nothing():
    name = Cs
    out_g, _l = _forward(name)
    with torch.no_grad():
        out, _l = _forward(name)
    for f in Projection._fields:
        t = getattr(out[-1], f)
        assert not t.requires_grad and t.grad_fn is None and torch.equal(t, getattr(out_g[-1], f).detach()), f
    # nothing extra is saved: once the outputs are dropped, a no_grad forward with the setting on holds on to exactly as much
    # device memory as one with it off (whatever the library keeps per thread between forwards is the same in both)
    del out_g, out, _l, t
    held = {}
    for on in (False, True, False, True):   # (each once to warm the caches, then the pair that is compared)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            out, leaves = _forward(name, return_projection=on)
        assert len(out) == 3 + on
        del out, leaves
        torch.cuda.synchronize()
        held[on] = torch.cuda.memory_allocated() - base
    print(f"held after a no_grad forward: off {held[False]} B, on {held[True]} B")
    assert held[True] == held[False]


def test_sync_free_graph_replay_equals_eager():
    name = Cs
    g = {f: t.to(DEV) for f, t in _g(name).items()}
    s, kw, leaves = _leaves(name)
    rs = _settings(name, s, leaves, list_capacity=40_000)
    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)
    rast = GaussianRasterizer(rs)
    keys = _inputs(name)

    def fwd_bwd():
        for t in list(leaves.values()) + [m2d]:
            t.grad = None
        p = rast(means2D=m2d, **kw)[-1]
        sum((getattr(p, f) * g[f]).sum() for f in FIELDS).backward()
        return p

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_p = fwd_bwd()
    g_grads = {k: leaves[k].grad for k in keys}
    with torch.no_grad():
        leaves["opacities"].mul_(0.8)
        leaves["means3D"].mul_(1.01)
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy().copy() for k, v in g_grads.items()}
    got_p = [t.detach().clone() for t in g_p]
    e = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}   # eager, exact mode, on the changed inputs
    p = GaussianRasterizer(_settings(name, s, e))(means2D=torch.zeros_like(e["means3D"]), **e)[-1]
    sum((getattr(p, f) * g[f]).sum() for f in FIELDS).backward()
    for a, b, f in zip(got_p, p, Projection._fields):
        assert torch.equal(a, b.detach()), f
    _close(got, _np_grads(e), keys, "graph replay")


# ---- 7. off is off -----------------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_projection_call(monkeypatch):
    name = A
    _P, W, H = pj.REF_CASES[name][:3]
    lib = _lib.load()
    calls = []
    dL = upstream_gradient(W, H, seed=2241).to(DEV)
    # one pixel's colour and depth: every record slot of the blend backward then receives ONE addend per Gaussian, so the sums do
    # not depend on the order of its float atomics and two backwards can be compared bit for bit (the full frame: within GRAD_RTOL)
    one = torch.zeros(3, H, W, device=DEV)
    one[:, H // 2, W // 2] = torch.tensor([0.7, -1.3, 0.4], device=DEV)
    pix = lambda o: (o[0] * one).sum() + 0.5 * o[2][H // 2, W // 2]
    frame = lambda o: (o[0] * dL).sum()
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_projection", lambda *a: calls.append("f") or 99)
        mp.setattr(lib, "ggr_projection_backward", lambda *a: calls.append("b") or 99)
        s, kw, leaves = _leaves(name)
        never = s.settings()._replace(sh_max_degree=3)   # a settings object that never heard of the keyword
        res = {}
        for tag, rs in (("never", never), ("off", never._replace(return_projection=False))):
            for loss in ("pix", "frame"):
                s, kw, leaves = _leaves(name, pose=True)
                r = rs._replace(viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"], campos=leaves["campos"],
                                tanfov=leaves["tanfov"])
                leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
                out = GaussianRasterizer(r)(means2D=leaves["means2D"], **kw)
                (pix if loss == "pix" else frame)(out).backward()
                res[tag, loss] = (out, _np_grads(leaves))
    assert not calls
    for loss in ("pix", "frame"):
        (o1, g1), (o2, g2) = res["never", loss], res["off", loss]
        assert len(o1) == len(o2) == 3 and all(torch.equal(a, b) for a, b in zip(o1, o2))
    g1, g2 = res["never", "pix"][1], res["off", "pix"][1]
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    assert all(np.any(g1[k]) for k in _inputs(name))
    _close(res["off", "frame"][1], res["never", "frame"][1], _inputs(name), "off, full frame")
    # on, with a loss that does not touch the projection: the same outputs in front, no backward call, the same gradients
    seen = []
    real = lib.ggr_projection_backward
    monkeypatch.setattr(lib, "ggr_projection_backward", lambda *a: seen.append(1) or real(*a))
    out_on, g_on = _run(name, {}, pose=True, more=pix)
    assert not seen and len(out_on) == 4 and all(torch.equal(a, b) for a, b in zip(out_on[:3], res["never", "pix"][0]))
    for k in g1:
        assert np.array_equal(g_on[k], g1[k]), k
