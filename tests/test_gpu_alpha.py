"""The accumulated-opacity output on the GPU (`-m gpu`): `return_alpha` / GgrForwardExtra.out_alpha, GgrBackwardExtra.

alpha = 1 − T, the T the colour multiplies bg by.  Checked: against the colour itself (zero colours over a white background),
against the C oracle's final T at full size, gradients against the composed torch reference (tests/alpha_reference.py),
the negation identity with the background term, an alpha-only loss in one cell (the zero-gradient skip), every mode's
contract, the call-site layer and a plain-C host.

"Bit-identical" is said of images, radii, depth and alpha.  Gradients of two runs are compared within rounding (rel-L2 < 2e-5,
as tests/test_gpu_list_hint.py does): the blend backward accumulates them with float atomics in varying order."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ggrt_official_amd
from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views
from ggrt_official_amd.synthetic import CONFIGS, make_scene, upstream_gradient
from tests.alpha_reference import rasterize_alpha
from tests.helpers import FLIP_FRACTION, FWD_ATOL, GRAD_RTOL_ALL, check_image, oracle_forward, record_metric, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alpha_grad(W, H, seed):
    return upstream_gradient(W, H, seed=seed)[0] * 2.0   # [H,W], the same scale as a colour channel's gradient


def _run(sc, g, dL, use_sh=True, use_cov=True, colors=None, pose=False, sh_max_degree=3, want_alpha=True, **extra):
    """GaussianRasterizer forward + backward of Σ g·alpha + Σ dL·colour (either may be None) on cuda:0; returns (color,
    radii, depth, alpha, grads) as numpy."""
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    means, op = leaf(s.means3D), leaf(s.opacities)
    m2d = torch.zeros_like(means, requires_grad=True)
    kw, leaves = {}, dict(means3D=means, opacities=op, means2D=m2d)
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(colors)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(s.scales)
        leaves["rotations"] = kw["rotations"] = leaf(s.rotations)
    rs = s.settings()._replace(sh_max_degree=sh_max_degree, return_alpha=want_alpha, **extra)
    if pose:
        view, proj, cam = leaf(s.viewmatrix), leaf(s.projmatrix), leaf(s.campos)
        rs = rs._replace(viewmatrix=view, projmatrix=proj, campos=cam)
        leaves.update(viewmatrix=view, projmatrix=proj, campos=cam)
    out = GaussianRasterizer(rs)(means3D=means, means2D=m2d, opacities=op, **kw)
    assert len(out) == (4 if want_alpha else 3)
    color, radii, depth = out[:3]
    alpha = out[3] if want_alpha else None
    loss = 0.0
    if dL is not None:
        loss = loss + (color * dL.to(DEV)).sum()
    if g is not None:
        loss = loss + (alpha * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    return n(color), n(radii), n(depth), n(alpha), grads


def _small(seed=301):
    sc = make_scene(20000, 176, 144, sh_degree=3, seed=seed)
    return sc, _alpha_grad(176, 144, seed + 1), upstream_gradient(176, 144, seed=seed + 2)


# ---- 1. alpha is 1 − T --------------------------------------------------------------------------------------------------
def test_alpha_is_one_minus_the_colour_of_black_splats_over_white():
    sc = make_scene(30000, 208, 160, sh_degree=0, seed=311)
    sc.bg = torch.ones(3)
    zero = torch.zeros(30000, 3)
    color, _, _, alpha, _ = _run(sc, _alpha_grad(208, 160, 1), None, use_sh=False, colors=zero)
    assert np.array_equal(alpha, (1.0 - color[0]).astype(np.float32))   # colour = 0 + T·1 exactly, so bit for bit
    assert alpha.max() > 0.9 and alpha.min() < alpha.max()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["C1", "C3"])
def test_alpha_matches_the_c_oracles_final_T(name):
    sc = make_scene(seed=0, **CONFIGS[name])
    st = oracle_forward(sc)
    s = sc.to(DEV)
    rs = s.settings()._replace(sh_max_degree=3, return_alpha=True)
    with torch.no_grad():
        color, radii, _, alpha = GaussianRasterizer(rs)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D),
                                                        opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)
    assert np.array_equal(radii.cpu().numpy(), st.radii)
    check_image(color.cpu().numpy(), st.color, tag=f"alpha:{name}")
    a, want = alpha.cpu().numpy(), 1.0 - st.final_T
    flips = float((np.abs(a - want) > FWD_ATOL).mean())
    record_metric(f"alpha:{name}", alpha_flip_fraction=flips, alpha_max_abs=float(np.abs(a - want).max()))
    assert flips <= FLIP_FRACTION, flips


# ---- 2. gradients against the composed reference ----------------------------------------------------------------------
CASES = [
    # P, W, H, D, use_sh, use_cov, antialiasing, colour loss too, seed
    (25000, 208, 160, 3, True, True, False, True, 321),
    (25000, 208, 160, 3, False, False, False, True, 322),
    (25000, 208, 160, 3, True, False, True, True, 323),
    (25000, 192, 128, 3, False, True, True, False, 324),
]


@pytest.mark.parametrize("P,W,H,D,use_sh,use_cov,aa,with_colour,seed", CASES)
def test_gradients_match_the_composed_torch_reference(P, W, H, D, use_sh, use_cov, aa, with_colour, seed):
    sc = make_scene(P, W, H, sh_degree=D, seed=seed)
    g = _alpha_grad(W, H, seed)
    dL = upstream_gradient(W, H, seed=seed + 50) if with_colour else None
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    leaf = lambda t: t.float().clone().requires_grad_(True)
    m, op = leaf(sc.means3D), leaf(sc.opacities)
    kw = dict(cov3D_precomp=leaf(sc.cov3D)) if use_cov else dict(scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    kw.update(dict(shs=leaf(sc.shs)) if use_sh else dict(colors_precomp=leaf(colors)))
    color, radii, _, alpha = rasterize_alpha(m, op, sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg, W, H, sc.tanfovx,
                                             sc.tanfovy, D, sh_cap=3, antialiasing=aa, **kw)
    loss = (alpha * g).sum() + ((color * dL).sum() if dL is not None else 0.0)
    loss.backward()
    ref = dict(means3D=m.grad, opacities=op.grad, **{k: v.grad for k, v in kw.items()})
    h_color, h_radii, _, h_alpha, grads = _run(sc, g, dL, use_sh=use_sh, use_cov=use_cov, colors=colors, antialiasing=aa)
    assert np.array_equal(h_radii, radii.numpy())
    check_image(h_alpha[None], alpha.detach().numpy()[None], name="alpha", tag=f"alpha:grad{seed}", psnr_min=100.0)
    for k, r in ref.items():
        if not with_colour and k in ("shs", "colors_precomp"):
            # alpha does not depend on the colours: none of their gradient here (the reference's is the rounding of two
            # blends' colour sums that cancel)
            assert not np.any(grads[k]), k
            continue
        e = rel_l2(grads[k], r.numpy())
        assert e <= GRAD_RTOL_ALL, f"grad {k}: rel-L2 {e:.3e}"


def test_camera_gradients_match_the_composed_reference():
    W, H = 160, 128
    sc = make_scene(12000, W, H, sh_degree=3, seed=331)
    g = _alpha_grad(W, H, 332)
    dL = upstream_gradient(W, H, seed=333)   # (campos reaches only the SH colours, which alpha does not depend on)
    leaf = lambda t: t.float().clone().requires_grad_(True)
    view, proj, cam = leaf(sc.viewmatrix), leaf(sc.projmatrix), leaf(sc.campos)
    color, _, _, alpha = rasterize_alpha(sc.means3D, sc.opacities, view, proj, cam, sc.bg, W, H, sc.tanfovx, sc.tanfovy, 3,
                                         shs=sc.shs, cov3D_precomp=sc.cov3D, sh_cap=3)
    ((alpha * g).sum() + (color * dL).sum()).backward()
    _, _, _, _, grads = _run(sc, g, dL, pose=True)
    for k, ref in (("viewmatrix", view.grad), ("projmatrix", proj.grad), ("campos", cam.grad)):
        r = rel_l2(grads[k], ref.numpy())
        assert r <= 2e-3, f"{k}: rel-L2 {r:.3e}"   # (the camera-gradient bar of tests/test_gpu_antialiasing.py)


def test_segmented_replay_of_long_lists():
    """A frame far below 4096 tiles whose lists span several checkpoint segments: the alpha seed enters every segment's
    re-entry (blend_bwd.hip), gradients as the composed reference's."""
    W, H = 80, 64
    sc = make_scene(30000, W, H, sh_degree=1, profile="B", seed=341)
    sc.opacities.mul_(0.5)    # faint splats: pixels stay unsaturated deep into the lists
    st = oracle_forward(sc, sh_cap=3)
    assert st.n_contrib.max() > 4 * 256, "the case is meant to keep several segments busy"
    g = _alpha_grad(W, H, 342)
    leaf = lambda t: t.float().clone().requires_grad_(True)
    m, op, sh, cov = leaf(sc.means3D), leaf(sc.opacities), leaf(sc.shs), leaf(sc.cov3D)
    _, _, _, alpha = rasterize_alpha(m, op, sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg, W, H, sc.tanfovx, sc.tanfovy,
                                     1, shs=sh, cov3D_precomp=cov, sh_cap=3)
    (alpha * g).sum().backward()
    _, _, _, _, grads = _run(sc, g, None)
    for k, r in (("means3D", m.grad), ("opacities", op.grad), ("cov3D_precomp", cov.grad)):
        e = rel_l2(grads[k], r.numpy())
        assert e <= GRAD_RTOL_ALL, f"grad {k}: rel-L2 {e:.3e}"


# ---- 3. the negation identity, no oracle ------------------------------------------------------------------------------
def test_alpha_gradients_are_minus_the_background_terms():
    """Zero colours: colour[0] with bg = (1,0,0) is T, alpha is 1 − T — their gradients are exact negatives."""
    W, H, P = 208, 160, 25000
    sc = make_scene(P, W, H, sh_degree=0, seed=351)
    sc.bg = torch.tensor([1.0, 0.0, 0.0])
    zero = torch.zeros(P, 3)
    g = _alpha_grad(W, H, 352)
    a = _run(sc, g, None, use_sh=False, colors=zero)
    dL = torch.zeros(3, H, W)
    dL[0] = g
    c = _run(sc, None, dL, use_sh=False, colors=zero, want_alpha=False)
    for k in ("means3D", "means2D", "opacities", "cov3D_precomp"):
        assert np.abs(a[4][k]).max() > 0, k
        r = rel_l2(a[4][k], -c[4][k])
        assert r < 2e-5, f"{k}: rel-L2 {r:.3e}"


# ---- 4. an alpha-only loss in one cell --------------------------------------------------------------------------------
def test_alpha_only_loss_in_one_cell_is_not_skipped():
    """dL/dcolour = 0 everywhere, dL/dalpha nonzero in one 2×2 cell: the zero-gradient window skip must keep that cell."""
    W, H = 192, 128
    sc = make_scene(15000, W, H, sh_degree=3, seed=361)
    g = torch.zeros(H, W)
    g[70:72, 101:103] = torch.tensor([[1.0, -0.5], [0.25, 2.0]])
    leaf = lambda t: t.float().clone().requires_grad_(True)
    m, op, sh, cov = leaf(sc.means3D), leaf(sc.opacities), leaf(sc.shs), leaf(sc.cov3D)
    _, _, _, alpha = rasterize_alpha(m, op, sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg, W, H, sc.tanfovx, sc.tanfovy,
                                     3, shs=sh, cov3D_precomp=cov, sh_cap=3)
    assert float(alpha.detach()[70:72, 101:103].min()) > 0.1
    (alpha * g).sum().backward()
    _, _, _, _, grads = _run(sc, g, torch.zeros(3, H, W))   # (an explicit zero colour gradient, as a masked loss gives)
    assert np.count_nonzero(op.grad.numpy()) > 0
    for k, r in (("means3D", m.grad), ("opacities", op.grad), ("cov3D_precomp", cov.grad)):
        assert np.abs(grads[k]).max() > 0, k
        e = rel_l2(grads[k], r.numpy())
        assert e <= GRAD_RTOL_ALL, f"grad {k}: rel-L2 {e:.3e}"
    assert not np.any(grads["shs"])


# ---- 5. every mode's contract -----------------------------------------------------------------------------------------
def _cams(s, V):
    view = torch.stack([s.viewmatrix.clone() for _ in range(V)])
    for v in range(V):   # (a small sideways shift per view)
        view[v, 3, 0] += 0.05 * v
    proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(V)])
    cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(V)])
    return view, proj, cam


def _views(sc, V, per_view=False):
    """V views of one scene, Σ g·alpha + Σ dL·colour: (colour, alpha, radii, dmeans, dop, dshs, dcov) — as one launch set
    or view by view (gradients summed by autograd)."""
    s = sc.to(DEV)
    view, proj, cam = _cams(s, V)
    bg = s.bg.reshape(1, 3).expand(V, 3).contiguous()
    tf = torch.tensor([[s.tanfovx, s.tanfovy]] * V, dtype=torch.float32, device=DEV)
    dL = torch.stack([upstream_gradient(s.width, s.height, seed=400 + v, device=DEV) for v in range(V)])
    g = torch.stack([_alpha_grad(s.width, s.height, 410 + v) for v in range(V)]).to(DEV)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    means, op, shs, cov = leaf(s.means3D), leaf(s.opacities), leaf(s.shs), leaf(s.cov3D)
    rs = s.settings()._replace(sh_max_degree=3, return_alpha=True)
    if per_view:
        cols, alphas, rads = [], [], []
        for v in range(V):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=bg[v])
            c, rad, _, a = GaussianRasterizer(r)(means3D=means, means2D=torch.zeros_like(means, requires_grad=True),
                                                 opacities=op, shs=shs, cov3D_precomp=cov)
            ((c * dL[v]).sum() + (a * g[v]).sum()).backward()
            cols.append(c.detach()); alphas.append(a.detach()); rads.append(rad)
        col, alpha, rad = torch.stack(cols), torch.stack(alphas), torch.stack(rads)
    else:
        col, rad, _, alpha = rasterize_views(means, op, view, proj, cam, bg, tf, rs, shs=shs, cov3D_precomp=cov)
        assert alpha.shape == (V, s.height, s.width)
        ((col * dL).sum() + (alpha * g).sum()).backward()
        col, alpha = col.detach(), alpha.detach()
    torch.cuda.synchronize()
    return col, alpha, rad, means.grad, op.grad, shs.grad, cov.grad


def test_launch_set_equals_per_view_calls():
    sc, _, _ = _small(421)
    a = _views(sc, 4)
    b = _views(sc, 4, per_view=True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for x, y in zip(a[3:], b[3:]):
        assert rel_l2(x.cpu().numpy(), y.cpu().numpy()) < 2e-5


def test_two_gaussian_sets_equal_per_view_calls():
    """num_sets > 1: two Gaussian sets of two views each against four per-view calls."""
    scs = [make_scene(8000, 160, 128, sh_degree=3, seed=430 + b).to(DEV) for b in range(2)]
    view, proj, cam = [], [], []
    for s in scs:
        v, p, c = _cams(s, 2)
        view.append(v); proj.append(p); cam.append(c)
    view, proj, cam = torch.cat(view), torch.cat(proj), torch.cat(cam)
    bg = torch.stack([scs[v // 2].bg for v in range(4)])
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 4, dtype=torch.float32, device=DEV)
    g = torch.stack([_alpha_grad(160, 128, 440 + v) for v in range(4)]).to(DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3, return_alpha=True)
    stk = lambda f: torch.stack([f(s) for s in scs]).detach().clone().requires_grad_(True)
    m, op = stk(lambda s: s.means3D), stk(lambda s: s.opacities)
    col, _, _, alpha = rasterize_views(m, op, view, proj, cam, bg, tf, rs, shs=stk(lambda s: s.shs),
                                       cov3D_precomp=stk(lambda s: s.cov3D))
    (alpha * g).sum().backward()
    for v in range(4):
        s = scs[v // 2]
        r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=bg[v], tanfovx=s.tanfovx,
                        tanfovy=s.tanfovy)
        mv, opv = s.means3D.clone().requires_grad_(True), s.opacities.clone().requires_grad_(True)
        c, _, _, a = GaussianRasterizer(r)(means3D=mv, means2D=torch.zeros_like(mv), opacities=opv, shs=s.shs,
                                           cov3D_precomp=s.cov3D)
        assert torch.equal(col[v].detach(), c.detach()) and torch.equal(alpha[v].detach(), a.detach()), v
        if v % 2 == 0:   # the set's gradient = the sum over its two views
            (a * g[v]).sum().backward()
            mv2, opv2 = s.means3D.clone().requires_grad_(True), s.opacities.clone().requires_grad_(True)
            r2 = r._replace(viewmatrix=view[v + 1], projmatrix=proj[v + 1], campos=cam[v + 1], bg=bg[v + 1])
            a2 = GaussianRasterizer(r2)(means3D=mv2, means2D=torch.zeros_like(mv2), opacities=opv2, shs=s.shs,
                                        cov3D_precomp=s.cov3D)[3]
            (a2 * g[v + 1]).sum().backward()
            b = v // 2
            assert rel_l2(m.grad[b].cpu().numpy(), (mv.grad + mv2.grad).cpu().numpy()) < 2e-5
            assert rel_l2(op.grad[b].cpu().numpy(), (opv.grad + opv2.grad).cpu().numpy()) < 2e-5


def test_scissor_window_equals_full_frame_and_zero_outside():
    sc, g, dL = _small(451)
    win = (40, 24, 150, 120)
    full = _run(sc, g, dL)
    cut = _run(sc, g, dL, scissor=win)
    x0, y0, x1, y1 = win
    tx0, ty0, tx1, ty1 = x0 // 16 * 16, y0 // 16 * 16, -(-x1 // 16) * 16, -(-y1 // 16) * 16
    assert np.array_equal(full[3][ty0:ty1, tx0:tx1], cut[3][ty0:ty1, tx0:tx1])
    assert np.array_equal(full[0][:, ty0:ty1, tx0:tx1], cut[0][:, ty0:ty1, tx0:tx1])
    outside = np.ones_like(cut[3], bool)
    outside[ty0:ty1, tx0:tx1] = False
    assert full[3][outside].max() > 0 and not np.any(cut[3][outside])


def test_inference_equals_training_forward():
    sc, g, dL = _small(461)
    s = sc.to(DEV)
    train = _run(sc, g, dL)
    with torch.no_grad():
        c, r, d, a = GaussianRasterizer(s.settings()._replace(sh_max_degree=3, return_alpha=True))(
            means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)
    for x, y in zip((c, r, d, a), train[:4]):
        assert np.array_equal(x.cpu().numpy(), y)


def test_a_missed_list_hint_is_repaired_as_exact_mode():
    P, W, H = 50_000, 320, 240
    small = make_scene(P, W, H, sh_degree=1, profile="B", seed=6)      # small splats: few list entries
    big = make_scene(P, W, H, sh_degree=1, profile="A", seed=7)        # same shape, several times the entries
    g, dL = _alpha_grad(W, H, 471), upstream_gradient(W, H, seed=472)
    prev = ggrt_official_amd.set_list_hint(False)
    try:
        want = _run(big, g, dL)
        ggrt_official_amd.set_list_hint(True)
        ggrt_official_amd.clear_list_hints()
        ggrt_official_amd.list_hint_stats(reset=True)
        _run(small, g, dL)                # notes the small N
        got = _run(big, g, dL)            # guess too small → repaired inside the call
        assert ggrt_official_amd.list_hint_stats()["missed"] == 1
        for x, y in zip(got[:4], want[:4]):
            assert np.array_equal(x, y)
        for k in want[4]:
            assert rel_l2(got[4][k], want[4][k]) < 2e-5, k
    finally:
        ggrt_official_amd.clear_list_hints()
        ggrt_official_amd.set_list_hint(prev)


def test_sync_free_graph_replay_equals_eager():
    sc, g, _ = _small(481)
    s = sc.to(DEV)
    g = g.to(DEV)
    rs = s.settings()._replace(list_capacity=400_000, sh_max_degree=3, return_alpha=True)
    means, shs, op, cov = [t.clone().requires_grad_() for t in (s.means3D, s.shs, s.opacities, s.cov3D)]
    m2d = torch.zeros_like(means, requires_grad=True)
    rast = GaussianRasterizer(rs)

    def fwd_bwd():
        for t in (means, shs, op, cov, m2d):
            t.grad = None
        _, radii, _, alpha = rast(means3D=means, means2D=m2d, opacities=op, shs=shs, cov3D_precomp=cov)
        (alpha * g).sum().backward()
        return alpha, radii

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_alpha, g_radii = fwd_bwd()
    g_grads = [means.grad, op.grad, cov.grad]
    with torch.no_grad():
        op.mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    got = [g_alpha.detach().clone(), g_radii.clone()] + [t.clone() for t in g_grads]
    e = [t.detach().clone().requires_grad_() for t in (means, shs, op, cov)]
    _, radii, _, alpha = GaussianRasterizer(s.settings()._replace(sh_max_degree=3, return_alpha=True))(
        means3D=e[0], means2D=torch.zeros_like(e[0]), opacities=e[2], shs=e[1], cov3D_precomp=e[3])
    (alpha * g).sum().backward()
    assert torch.equal(got[0], alpha.detach()) and torch.equal(got[1], radii)
    for a, b in zip(got[2:], [e[0].grad, e[2].grad, e[3].grad]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 2e-5


# ---- 6. off = as before -----------------------------------------------------------------------------------------------
def test_off_is_bit_identical_to_the_entry_points_without_extras(monkeypatch):
    """return_alpha=False through the `_ext` entry points (NULL extras) = the calls without extras; and with alpha on, the
    colour, radii and depth are those of the call without it."""
    lib = _lib.load()
    sc, g, dL = _small(491)
    got = _run(sc, None, dL, want_alpha=False)
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_forward_ext", lambda st, opt, ex, fin, fout, cb, ctx, stream:
                   lib.ggr_forward_opt(st, opt, fin, fout, cb, ctx, stream) if ex is None else 99)
        mp.setattr(lib, "ggr_backward_ext", lambda st, ex, bin_, bout, stream:
                   lib.ggr_backward(st, bin_, bout, stream) if ex is None else 99)
        ref = _run(sc, None, dL, want_alpha=False)
    for a, b in zip(got[:3], ref[:3]):
        assert np.array_equal(a, b)
    for k in ref[4]:
        assert rel_l2(got[4][k], ref[4][k]) < 2e-5, k
    on = _run(sc, g, dL)
    for a, b in zip(on[:3], ref[:3]):
        assert np.array_equal(a, b)
    # a launch set
    s = sc.to(DEV)
    view, proj, cam = _cams(s, 3)
    bg = s.bg.reshape(1, 3).expand(3, 3).contiguous()
    tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 3, dtype=torch.float32, device=DEV)
    rs = s.settings()._replace(sh_max_degree=3)
    call = lambda r: rasterize_views(s.means3D, s.opacities, view, proj, cam, bg, tf, r, shs=s.shs, cov3D_precomp=s.cov3D)
    with torch.no_grad():
        off = call(rs)
        with monkeypatch.context() as mp:
            mp.setattr(lib, "ggr_forward_views_ext", lambda st, opt, ex, vw, fin, fout, cb, ctx, stream:
                       lib.ggr_forward_views_opt(st, opt, vw, fin, fout, cb, ctx, stream) if ex is None else 99)
            plain = call(rs)
        on_v = call(rs._replace(return_alpha=True))
    assert len(off) == 3 and len(on_v) == 4
    for a, b, c in zip(off, plain, on_v[:3]):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- 7. the call-site layer -------------------------------------------------------------------------------------------
def test_decoder_alpha_equals_per_view_rasterizer_calls():
    from ggrt_official_amd import splatting as S
    gen = torch.Generator().manual_seed(501)
    b, v, n, d_sh, h, w = 2, 3, 4000, 16, 96, 128
    ext = torch.eye(4).repeat(b, v, 1, 1)
    ext[..., 0, 3] = torch.linspace(-0.2, 0.2, v)
    K = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    means = torch.randn(b, n, 3, generator=gen) * torch.tensor([0.6, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(b, n, 3, 3, generator=gen) * 0.05
    cov = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3)
    harm = torch.randn(b, n, 3, d_sh, generator=gen) * 0.3
    opac = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    to = lambda t: t.to(DEV)
    gs = S.Gaussians(to(means), to(cov), to(harm), to(opac))
    dec = S.DecoderSplattingCUDA(sh_max_degree=4).to(DEV)
    args = (gs, to(ext), to(K), to(near), to(far), (h, w))
    with torch.no_grad():
        out = dec(*args, depth_mode="depth", return_alpha=True)
        ref = dec(*args, depth_mode="depth")
        assert out.alpha.shape == (b, v, h, w) and ref.alpha is None
        assert torch.equal(out.color, ref.color) and torch.equal(out.depth, ref.depth)
        # per view: the same call site with one rasterizer call per view (launch sets off) — bit for bit
        per_view = S.render_views_fused(to(ext).flatten(0, 1), to(K).flatten(0, 1), to(near).flatten(), to(far).flatten(),
                                        (h, w), torch.zeros(b * v, 3, device=DEV), gs, [k // v for k in range(b * v)],
                                        "depth", batched=False, sh_max_degree=4, return_alpha=True)
        assert len(per_view) == 3
        assert torch.equal(out.alpha, per_view[2].reshape(b, v, h, w))
        assert torch.equal(out.color, per_view[0].reshape(b, v, 3, h, w))
        # the unfused call site (render_color_and_depth: the reference's torch pre-processing) returns alpha too
        slow = S.DecoderSplattingCUDA(sh_max_degree=4, fused_inputs=False).to(DEV)
        o2, r2 = slow(*args, depth_mode="depth", return_alpha=True), slow(*args, depth_mode="depth")
        assert torch.equal(o2.color, r2.color) and torch.equal(o2.depth, r2.depth) and r2.alpha is None
        assert float((o2.alpha - out.alpha).abs().mean()) < 1e-5
    # differentiable through the decoder
    leaf = gs.opacities.clone().requires_grad_(True)
    o = dec(S.Gaussians(gs.means, gs.covariances, gs.harmonics, leaf), *args[1:], return_alpha=True)
    o.alpha.sum().backward()
    assert float(leaf.grad.abs().max()) > 0


# ---- 8. a plain-C host ------------------------------------------------------------------------------------------------
def test_c_host_forward_ext_backward_ext_known_answer(tmp_path):
    from ggrt_official_amd import _build
    _build.build_library()
    src, libdir = os.path.join(ROOT, "tests", "c_abi", "alpha_smoke.c"), os.path.join(ROOT, "ggrt_official_amd")
    exe = str(tmp_path / "alpha_smoke")
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-D__HIP_PLATFORM_AMD__", src,
           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-L" + libdir, "-L/opt/rocm/lib", "-lggr_raster",
           "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "C ABI ALPHA OK" in r.stdout, r.stdout
