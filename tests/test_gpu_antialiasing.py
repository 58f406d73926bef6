"""Anti-aliased rasterization on the GPU (`-m gpu`): upstream's `antialiasing` setting through GgrForwardOptions.

Off changes nothing; on, every stage but the opacity stays what it is, the images and gradients meet the composed torch
reference (tests/aa_reference.py), and every mode of the rasterizer keeps its contract.

"Bit-identical" is said of images, radii and depth.  Gradients are compared within rounding (rel-L2 < 2e-5, as
tests/test_gpu_list_hint.py does): the blend backward accumulates them with float atomics, whose order — and hence the last
bits — differs between two runs of the very same call."""
import ggrt_official_amd.rasterizer as R
import ctypes

import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views
from ggrt_official_amd.rasterizer import debug_forward_state
from ggrt_official_amd.synthetic import make_scene, upstream_gradient
from tests.aa_reference import AA_MIN_RATIO, rasterize_aa
from tests.helpers import GRAD_RTOL_ALL, check_image, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(sc, dL, aa, use_sh=True, use_cov=True, colors=None, pose=False, sh_max_degree=3, **extra):
    """GaussianRasterizer forward + backward on cuda:0; returns (color, radii, depth, grads) as numpy."""
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
    rs = s.settings()._replace(sh_max_degree=sh_max_degree, antialiasing=aa, **extra)
    if pose:
        view, proj, cam = leaf(s.viewmatrix), leaf(s.projmatrix), leaf(s.campos)
        rs = rs._replace(viewmatrix=view, projmatrix=proj, campos=cam)
        leaves.update(viewmatrix=view, projmatrix=proj, campos=cam)
    color, radii, depth = GaussianRasterizer(rs)(means3D=means, means2D=m2d, opacities=op, **kw)
    (color * dL.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in leaves.items()}
    return color.detach().cpu().numpy(), radii.cpu().numpy(), depth.detach().cpu().numpy(), grads


def _sub_pixel(sc, factor=1e-3):
    """The same scene with every covariance shrunk: most Gaussians sub-pixel (s ≪ 1), the smallest under the clamp."""
    sc.cov3D = sc.cov3D * factor
    sc.cov3D[::7] *= 1e-6
    sc.scales = sc.scales * factor ** 0.5
    return sc


def test_off_is_bit_identical_to_the_entry_points_without_options(monkeypatch):
    """antialiasing=False through ggr_forward_opt / ggr_forward_views_opt = ggr_forward / ggr_forward_views, every output
    and every gradient, one view and a launch set."""
    lib = _lib.load()
    sc = make_scene(20000, 192, 144, sh_degree=3, seed=101)
    dL = upstream_gradient(192, 144, seed=102)
    got = _run(sc, dL, False)
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_forward_opt", lambda st, opt, fin, fout, cb, ctx, stream:
                   lib.ggr_forward(st, fin, fout, cb, ctx, stream))
        ref = _run(sc, dL, False)
    for a, b in zip(got[:3], ref[:3]):
        assert np.array_equal(a, b)
    for k in ref[3]:
        assert rel_l2(got[3][k], ref[3][k]) < 2e-5, k
    g_v, r_v = _views(sc, 3, False), None
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_forward_views_opt", lambda st, opt, vw, fin, fout, cb, ctx, stream:
                   lib.ggr_forward_views(st, vw, fin, fout, cb, ctx, stream))
        r_v = _views(sc, 3, False)
    assert torch.equal(g_v[0], r_v[0]) and torch.equal(g_v[1], r_v[1])
    for a, b in zip(g_v[2:], r_v[2:]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 2e-5


def _cams(sc, V):
    s = sc.to(DEV)
    view = torch.stack([s.viewmatrix.clone() for _ in range(V)])
    for v in range(V):   # (a small sideways shift per view)
        view[v, 3, 0] += 0.05 * v
    proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(V)])
    cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(V)])
    return view, proj, cam


def _views(sc, V, aa, per_view=False):
    """V views of one scene: (images, radii, dmeans, dop, dshs, dcov) — as one launch set, or view by view (summed)."""
    s = sc.to(DEV)
    view, proj, cam = _cams(sc, V)
    bg = s.bg.reshape(1, 3).expand(V, 3).contiguous()
    tf = torch.tensor([[s.tanfovx, s.tanfovy]] * V, dtype=torch.float32, device=DEV)
    dL = torch.stack([upstream_gradient(s.width, s.height, seed=200 + v, device=DEV) for v in range(V)])
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    means, op, shs, cov = leaf(s.means3D), leaf(s.opacities), leaf(s.shs), leaf(s.cov3D)
    rs = s.settings()._replace(sh_max_degree=3, antialiasing=aa)
    if per_view:
        cols, rads = [], []
        for v in range(V):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=bg[v])
            c, rad, _ = GaussianRasterizer(r)(means3D=means, means2D=torch.zeros_like(means, requires_grad=True),
                                              opacities=op, shs=shs, cov3D_precomp=cov)
            (c * dL[v]).sum().backward()
            cols.append(c.detach())
            rads.append(rad)
        col, rad = torch.stack(cols), torch.stack(rads)
    else:
        col, rad, _ = rasterize_views(means, op, view, proj, cam, bg, tf, rs, shs=shs, cov3D_precomp=cov)
        (col * dL).sum().backward()
        col = col.detach()
    torch.cuda.synchronize()
    return col, rad, means.grad, op.grad, shs.grad, cov.grad


def test_anti_aliased_frames_keep_their_own_list_hints():
    import ggrt_official_amd
    sc, dL = _small()
    prev = ggrt_official_amd.set_list_hint(True)
    try:
        ggrt_official_amd.clear_list_hints()
        _run(sc, dL, True)
        key = (0, sc.means3D.shape[0], sc.width, sc.height, 1, None)
        assert R._capacity_guess(key) == (0, 0)                       # the default mode's history is untouched …
        assert R._capacity_guess(key + ("antialiasing",))[0] > 0      # … the anti-aliased frame has its own
    finally:
        ggrt_official_amd.clear_list_hints()
        ggrt_official_amd.set_list_hint(prev)


def test_stages_only_the_opacity_changes():
    sc = _sub_pixel(make_scene(30000, 208, 160, sh_degree=3, seed=111), 1e-2).to(DEV)
    rs = sc.settings()._replace(reference_rects=True, sh_max_degree=3)
    off = debug_forward_state(sc.means3D, sc.opacities, rs, shs=sc.shs, cov3D_precomp=sc.cov3D)
    on = debug_forward_state(sc.means3D, sc.opacities, rs._replace(antialiasing=True), shs=sc.shs, cov3D_precomp=sc.cov3D)
    for k in ("radii", "xy", "depth", "point_list", "ranges", "tiles_touched"):
        assert torch.equal(on[k], off[k]), k
    assert torch.equal(on["conic_opacity"][:, :3], off["conic_opacity"][:, :3])
    vis = on["radii"] > 0
    # opacity · s in float64, s from the record's own conic (the dilated 2D covariance it inverts)
    c = on["conic_opacity"][vis, :3].double()
    dc = c[:, 0] * c[:, 2] - c[:, 1] ** 2
    a, b, cc = c[:, 2] / dc, -c[:, 1] / dc, c[:, 0] / dc
    ratio = ((a - 0.3) * (cc - 0.3) - b * b) / (a * cc - b * b)
    s = torch.sqrt(torch.clamp(ratio, min=AA_MIN_RATIO))
    want = sc.opacities.reshape(-1)[vis].double() * s
    got = on["conic_opacity"][vis, 3].double()
    rel = ((got - want).abs() / want).cpu()
    well = (ratio > 0.05).cpu()   # (below, the float64 value taken from the fp32 conic itself carries the cancellation of det0)
    assert float(rel[well].max()) < 8 * 2.0 ** -24 * 8, float(rel[well].max())
    assert float(rel.median()) < 4 * 2.0 ** -24
    assert float(s.min()) < 0.1 and bool((ratio <= AA_MIN_RATIO).any())   # sub-pixel and clamped ones are there


CASES = [
    # P, W, H, D, profile, cap, use_sh, use_cov, sub-pixel, seed
    (30000, 208, 160, 3, "A", 3, True, True, False, 121),
    (30000, 208, 160, 4, "B", 4, True, True, False, 122),
    (25000, 192, 128, 3, "A", 3, False, False, False, 123),
    (30000, 208, 160, 3, "A", 3, True, True, True, 124),
    (30000, 208, 160, 4, "B", 3, True, False, True, 125),
]


@pytest.mark.parametrize("P,W,H,D,profile,cap,use_sh,use_cov,sub,seed", CASES)
def test_matches_the_composed_torch_reference(P, W, H, D, profile, cap, use_sh, use_cov, sub, seed):
    sc = make_scene(P, W, H, sh_degree=D, profile=profile, seed=seed)
    if sub:
        sc = _sub_pixel(sc)
    dL = upstream_gradient(W, H, seed=seed)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    leaf = lambda t: t.float().clone().requires_grad_(True)
    m, op = leaf(sc.means3D), leaf(sc.opacities)
    kw = dict(cov3D_precomp=leaf(sc.cov3D)) if use_cov else dict(scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    kw.update(dict(shs=leaf(sc.shs)) if use_sh else dict(colors_precomp=leaf(colors)))
    color, radii, depth, pre = rasterize_aa(m, op, sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg, W, H, sc.tanfovx,
                                            sc.tanfovy, D, sh_cap=cap, **kw)
    (color * dL).sum().backward()
    ref = dict(means3D=m.grad, opacities=op.grad, **{k: v.grad for k, v in kw.items()})
    h_color, h_radii, h_depth, grads = _run(sc, dL, True, use_sh=use_sh, use_cov=use_cov, colors=colors,
                                            sh_max_degree=cap)
    assert np.array_equal(h_radii, radii.numpy())
    tag = f"aa:{profile}{D}cap{cap}{'sub' if sub else ''}"
    check_image(h_color, color.detach().numpy(), tag=tag, psnr_min=100.0)
    if sub:
        assert float((pre["aa_scale"][pre["visible"]] < 0.2).float().mean()) > 0.3
    for k, g in ref.items():
        r = rel_l2(grads[k], g.numpy())
        assert r <= GRAD_RTOL_ALL, f"grad {k}: rel-L2 {r:.3e}"


def test_camera_gradients_match_torch_autograd():
    W, H = 160, 128
    sc = _sub_pixel(make_scene(12000, W, H, sh_degree=3, seed=131), 3e-2)
    dL = upstream_gradient(W, H, seed=132)
    leaf = lambda t: t.float().clone().requires_grad_(True)
    view, proj, cam = leaf(sc.viewmatrix), leaf(sc.projmatrix), leaf(sc.campos)
    color, _, _, _ = rasterize_aa(sc.means3D, sc.opacities, view, proj, cam, sc.bg, W, H, sc.tanfovx, sc.tanfovy, 3,
                                  shs=sc.shs, cov3D_precomp=sc.cov3D, sh_cap=3)
    (color * dL).sum().backward()
    _, _, _, grads = _run(sc, dL, True, pose=True)
    for k, ref in (("viewmatrix", view.grad), ("projmatrix", proj.grad), ("campos", cam.grad)):
        r = rel_l2(grads[k], ref.numpy())
        assert r <= 2e-3, f"{k}: rel-L2 {r:.3e}"


def _small():
    return _sub_pixel(make_scene(20000, 192, 144, sh_degree=3, seed=141), 3e-2), upstream_gradient(192, 144, seed=142)


def test_tight_rects_equal_reference_rects():
    sc, dL = _small()
    a = _run(sc, dL, True)
    b = _run(sc, dL, True, reference_rects=True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for k in a[3]:
        assert rel_l2(a[3][k], b[3][k]) < 2e-5, k


@pytest.mark.parametrize("V", [1, 3])
def test_launch_set_equals_per_view_calls(V):
    sc, _ = _small()
    a = _views(sc, V, True)
    b = _views(sc, V, True, per_view=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert rel_l2(x.cpu().numpy(), y.cpu().numpy()) < 1e-5


def test_two_gaussian_sets_equal_per_view_calls():
    """num_sets > 1: two Gaussian sets of two views each against four per-view calls (images bit-identical)."""
    scs = [_sub_pixel(make_scene(8000, 160, 128, sh_degree=3, seed=150 + b), 3e-2).to(DEV) for b in range(2)]
    view, proj, cam = [], [], []
    for sc in scs:
        v, p, c = _cams(sc, 2)
        view.append(v); proj.append(p); cam.append(c)
    view, proj, cam = torch.cat(view), torch.cat(proj), torch.cat(cam)
    bg = torch.stack([scs[v // 2].bg for v in range(4)])
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 4, dtype=torch.float32, device=DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3, antialiasing=True)
    st = lambda f: torch.stack([f(s) for s in scs])
    with torch.no_grad():
        col, _, _ = rasterize_views(st(lambda s: s.means3D), st(lambda s: s.opacities), view, proj, cam, bg, tf, rs,
                                    shs=st(lambda s: s.shs), cov3D_precomp=st(lambda s: s.cov3D))
        for v in range(4):
            s = scs[v // 2]
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=bg[v], tanfovx=s.tanfovx,
                            tanfovy=s.tanfovy)
            c, _, _ = GaussianRasterizer(r)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                            shs=s.shs, cov3D_precomp=s.cov3D)
            assert torch.equal(col[v], c), v


def test_scissor_window_equals_full_frame():
    sc, dL = _small()
    win = (40, 24, 150, 120)
    full = _run(sc, dL, True)
    cut = _run(sc, dL, True, scissor=win)
    x0, y0, x1, y1 = win
    tx0, ty0, tx1, ty1 = x0 // 16 * 16, y0 // 16 * 16, -(-x1 // 16) * 16, -(-y1 // 16) * 16
    assert np.array_equal(full[0][:, ty0:ty1, tx0:tx1], cut[0][:, ty0:ty1, tx0:tx1])


def test_inference_equals_training_forward():
    sc, dL = _small()
    s = sc.to(DEV)
    rs = s.settings()._replace(sh_max_degree=3, antialiasing=True)
    train = _run(sc, dL, True)
    with torch.no_grad():
        c, r, d = GaussianRasterizer(rs)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                         shs=s.shs, cov3D_precomp=s.cov3D)
    assert np.array_equal(c.cpu().numpy(), train[0]) and np.array_equal(r.cpu().numpy(), train[1])


def test_sync_free_graph_replay_equals_eager():
    sc, _ = _small()
    s = sc.to(DEV)
    dL = upstream_gradient(s.width, s.height, device=DEV)
    rs = s.settings()._replace(list_capacity=400_000, sh_max_degree=3, antialiasing=True)
    means, shs, op, cov = [t.clone().requires_grad_() for t in (s.means3D, s.shs, s.opacities, s.cov3D)]
    m2d = torch.zeros_like(means, requires_grad=True)
    rast = GaussianRasterizer(rs)

    def fwd_bwd():
        for t in (means, shs, op, cov, m2d):
            t.grad = None
        color, radii, _ = rast(means3D=means, means2D=m2d, opacities=op, shs=shs, cov3D_precomp=cov)
        color.backward(dL)
        return color, radii

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_color, g_radii = fwd_bwd()
    g_grads = [means.grad, shs.grad, op.grad, cov.grad]
    with torch.no_grad():
        op.mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    got = [g_color.clone(), g_radii.clone()] + [g.clone() for g in g_grads]
    e = [t.detach().clone().requires_grad_() for t in (means, shs, op, cov)]
    color, radii, _ = GaussianRasterizer(s.settings()._replace(sh_max_degree=3, antialiasing=True))(
        means3D=e[0], means2D=torch.zeros_like(e[0]), opacities=e[2], shs=e[1], cov3D_precomp=e[3])
    color.backward(dL)
    assert torch.equal(got[0], color.detach()) and torch.equal(got[1], radii)
    for a, b in zip(got[2:], [t.grad for t in e]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


def test_fused_colour_and_depth_pass():
    """render_color_and_depth (one rasterization, depth as the 4th feature) = render_cuda + render_depth_cuda under AA."""
    from ggrt_official_amd import splatting as S
    g = torch.Generator().manual_seed(161)
    b, n = 2, 3000
    ext = torch.eye(4).repeat(b, 1, 1)
    ext[:, :3, 3] = torch.tensor([[0.0, 0.0, -2.0], [0.1, 0.0, -2.2]])
    K = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, 1, 1)
    near, far = torch.full((b,), 0.5), torch.full((b,), 50.0)
    means = torch.randn(b, n, 3, generator=g) * 0.5
    A = torch.randn(b, n, 3, 3, generator=g) * 0.01
    cov = A @ A.transpose(-1, -2) + 1e-6 * torch.eye(3)
    sh = torch.randn(b, n, 3, 16, generator=g) * 0.3
    op = torch.rand(b, n, generator=g)
    t = lambda x: x.to(DEV)
    bg = torch.zeros(b, 3, device=DEV)
    args = (t(ext), t(K), t(near), t(far), (96, 128))
    col, dep = S.render_color_and_depth(*args, bg, t(means), t(cov), t(sh), t(op), "depth", sh_max_degree=3,
                                        antialiasing=True)
    col2 = S.render_cuda(*args, bg, t(means), t(cov), t(sh), t(op), sh_max_degree=3, antialiasing=True)
    dep2 = S.render_depth_cuda(*args, t(means), t(cov), t(op), mode="depth", antialiasing=True)
    col0 = S.render_cuda(*args, bg, t(means), t(cov), t(sh), t(op), sh_max_degree=3)
    assert torch.equal(col, col2)
    assert float((dep - dep2).abs().max()) <= 1e-5 * float(dep2.abs().max())
    assert not torch.equal(col, col0)   # (the keyword reaches the kernels)


def test_nan_opacity_takes_no_part():
    sc, dL = _small()
    sc.opacities = sc.opacities.clone()
    sc.opacities[5] = float("nan")
    col, radii, _, grads = _run(sc, dL, True)
    assert radii[5] == 0 and np.isfinite(col).all()
    for k in ("means3D", "opacities", "shs", "cov3D_precomp"):
        assert np.isfinite(grads[k]).all() and not grads[k][5].any(), k


@pytest.mark.timeout(900)
def test_full_size_c3():
    """C3 (1 M Gaussians, 1920×1080): the anti-aliased forward + backward completes; its tight-rect lists are no longer than
    without; a launch set's images equal its per-view calls."""
    from ggrt_official_amd.rasterizer import last_forward_status
    from ggrt_official_amd.synthetic import CONFIGS
    sc = make_scene(**CONFIGS["C3"], seed=0)
    dL = upstream_gradient(sc.width, sc.height, seed=3)
    c_off = _run(sc, dL, False)
    n_off = last_forward_status()[0]
    c_on = _run(sc, dL, True)
    n_on = last_forward_status()[0]
    assert 0 < n_on <= n_off, (n_on, n_off)
    assert np.isfinite(c_on[0]).all() and all(np.isfinite(g).all() for g in c_on[3].values())
    assert not np.array_equal(c_on[0], c_off[0])
    a = _views(sc, 2, True)
    b = _views(sc, 2, True, per_view=True)
    assert torch.equal(a[0], b[0])
