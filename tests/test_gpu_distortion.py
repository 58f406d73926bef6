"""The distortion pass on the GPU (`-m gpu`): `return_distortion` / ggr_distortion_forward / ggr_distortion_backward.

The scene (tests/distortion_reference.py `clustered_scene`): a 40×24 frame — 3×2 tiles, ragged right and bottom — of 700
Gaussians pulled towards tile (1, 0), whose list exceeds 512 entries (three LDS batches); pixels there stop early, pixels near
the edges run to the end of their lists.  tests/test_distortion_reference.py asserts these conditions on the reference, and
`test_the_scene_reaches_the_long_paths_on_the_gpu` on the product's own (tighter) lists.

Bars.  Planes: helpers.check_image — the image bar of the feature planes (|Δ| ≤ 1e-4·peak but for 5e-5 of the pixels, peak-
normalised PSNR ≥ 110 dB).  The float64 reference against its own float32 run on this scene differs by 4.6e-7 at a peak of 1.94
(tests/test_distortion_reference.py), far inside the bar, so the bar is kept as it is.  Gradients: helpers.check_grads as it is —
rel-L2 ≤ 1e-3 over all rows and ≤ GRAD_RTOL (2e-5) once the flip rule's rows are set aside (none at 700 rows: the rule is
proportional, so here 2e-5 holds over all rows); the camera tensors at the 1e-3 of the existing camera-gradient tests.

"Bit-identical" is said of planes.  Gradients of two runs are compared within rounding: they are accumulated with float atomics
in varying order."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views
from ggrt_official_amd.synthetic import make_scene, upstream_gradient
from tests import distortion_reference as dr
from tests.helpers import GRAD_RTOL, GRAD_RTOL_ALL, check_grads, check_image, rel_l2
from tests.test_gpu_alpha import _cams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, P = dr.GPU_W, dr.GPU_H, dr.GPU_P
K = 4

_cache = {}


def _scene():
    if "scene" not in _cache:
        _cache["scene"] = dr.clustered_scene()
    return _cache["scene"]


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _gq(seed=1321):
    """[H,W] upstream gradient of the plane; the four left-most columns exactly zero (those pixels take no entry in the backward)"""
    g = _rand(H, W, seed=seed) / (H * W)
    g[:, :4] = 0.0
    return g


def _extras(seed=1330):
    """what the mixed loss adds: gradients of colour, depth, alpha and K feature planes, and the per-Gaussian features"""
    return dict(dL=upstream_gradient(W, H, seed=seed), gD=_rand(H, W, seed=seed + 1) / (10.0 * H * W),
                gA=_rand(H, W, seed=seed + 2) / (H * W), gF=_rand(K, H, W, seed=seed + 3) / (3.0 * H * W),
                feats=torch.rand(P, K, generator=torch.Generator().manual_seed(seed + 4)) * 2.0 - 0.5)


# the two input forms of case 1: between them every gradient the depth plane's reaches
FORMS = {
    "sh_cov_viewz_pose": dict(use_sh=True, use_cov=True, aux=False, pose=True),
    "colours_scale_rot_aux": dict(use_sh=False, use_cov=False, aux=True, pose=False),
}


def _colors():
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(1340))


def _aux(sc):
    """a depth value that is not view z, but monotone in it (so the ordered form is the |·| form)"""
    return (sc.means3D[:, 2] * 0.5 + 1.0).sqrt().contiguous()


def _loss(out, gQ, mixed):
    loss = (out["distortion"] * gQ).sum()
    if mixed is not None:
        loss = loss + (out["color"] * mixed["dL"]).sum() + (out["depth"] * mixed["gD"]).sum() + \
            (out["alpha"] * mixed["gA"]).sum() + (out["features"] * mixed["gF"]).sum()
    return loss


def _run(sc, gQ, mixed=None, use_sh=True, use_cov=True, aux=None, pose=False, distortion=True, feats=None, gF=None, **extra):
    """Forward + backward on cuda:0 → (planes by name as numpy, grads).  `mixed`: the `_extras` dict of the mixed loss (switches
    alpha and features on); `feats` / `gF` alone: features in the loss without the rest."""
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    means, op = leaf(s.means3D), leaf(s.opacities)
    kw, leaves = {}, dict(means3D=means, opacities=op)
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(_colors())
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(s.scales)
        leaves["rotations"] = kw["rotations"] = leaf(s.rotations)
    if aux is not None:
        leaves["aux"] = kw["aux_precomp"] = leaf(aux)
    rs = s.settings()._replace(sh_max_degree=3, return_distortion=distortion, return_alpha=mixed is not None, **extra)
    if pose:
        view, proj, cam = leaf(s.viewmatrix), leaf(s.projmatrix), leaf(s.campos)
        rs = rs._replace(viewmatrix=view, projmatrix=proj, campos=cam)
        leaves.update(viewmatrix=view, projmatrix=proj, campos=cam)
    if mixed is not None:
        feats = mixed["feats"]
    if feats is not None:
        leaves["features"] = kw["features_precomp"] = leaf(feats)
    tup = GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means, requires_grad=True), opacities=op, **kw)
    names = ["color", "radii", "depth"] + (["alpha"] if mixed is not None else []) + (["features"] if feats is not None else []) + \
        (["distortion"] if distortion else [])
    assert len(tup) == len(names)
    out = dict(zip(names, tup))
    to = lambda t: t.to(DEV)
    if distortion:
        loss = _loss(out, to(gQ), None if mixed is None else {k: to(v) for k, v in mixed.items()})
    else:
        loss = (out["color"] * to(mixed["dL"])).sum() if mixed is not None else 0.0
    if gF is not None and mixed is None:
        loss = loss + (out["features"] * to(gF)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (np.zeros(tuple(v.shape), np.float32) if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, grads


def _reference(form, mixed):
    """float64 reference planes and gradients of one input form under one loss — computed once per process, read only"""
    key = (form, mixed)
    if key not in _cache:
        f = FORMS[form]
        sc = _scene()
        kw = dr.scene_inputs(sc, torch.float64, f["use_sh"], f["use_cov"], _colors(), leaf=True)
        aux = _aux(sc).double().requires_grad_(True) if f["aux"] else None
        ex = {k: v.double() for k, v in _extras().items()} if mixed else None
        feats = ex["feats"].clone().requires_grad_(True) if mixed else None
        out = dr.run_reference(sc, kw, aux=aux, features=feats)
        _loss(out, _gq().double(), ex).backward()
        names = dict(kw, aux=aux, features=feats)
        grads = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy()) for k, v in names.items() if v is not None}
        planes = {k: out[k].detach().numpy() for k in ("color", "depth", "alpha", "distortion")}
        _cache[key] = (planes, grads, out["radii"].numpy())
    return _cache[key]


# ---- the scene's conditions, on the product's own lists ---------------------------------------------------------------------------
def test_the_scene_reaches_the_long_paths_on_the_gpu():
    import ggrt_official_amd.rasterizer as R
    out, _ = _run(_scene(), _gq())
    assert R.last_forward_binning()[1] > 512, "no tile list of three LDS batches"
    q = out["distortion"]
    assert q.shape == (H, W) and float(q.max()) > 1.0 and float(q.min()) >= 0.0


# ---- 1. plane and all gradients against the float64 reference ---------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["distortion_only", "mixed_loss"])
@pytest.mark.parametrize("form", list(FORMS))
def test_plane_and_gradients_match_the_float64_reference(form, mixed):
    f = FORMS[form]
    sc = _scene()
    planes, ref, radii = _reference(form, mixed)
    out, grads = _run(sc, _gq(), _extras() if mixed else None, use_sh=f["use_sh"], use_cov=f["use_cov"],
                      aux=_aux(sc) if f["aux"] else None, pose=f["pose"])
    assert np.array_equal(out["radii"], radii)
    d = np.abs(out["distortion"].astype(np.float64) - planes["distortion"])
    print(f"{form} mixed={mixed}: distortion peak {planes['distortion'].max():.3f}, max |Δ| {d.max():.3e}")
    check_image(out["distortion"], planes["distortion"], name="distortion", tag=f"dist:{form}")
    check_image(out["depth"], planes["depth"], name="depth", tag=f"dist:depth:{form}")
    keys = ["means3D", "opacities"] + (["cov3D_precomp"] if f["use_cov"] else ["scales", "rotations"]) + \
        (["aux"] if f["aux"] else []) + (["viewmatrix", "projmatrix", "campos"] if f["pose"] else []) + \
        (["features"] if mixed else [])
    for k in keys:
        print(f"{form} mixed={mixed} grad {k}: rel-L2 {rel_l2(grads[k], ref[k]):.3e}, |ref| {np.linalg.norm(ref[k]):.3e}")
    assert all(np.linalg.norm(ref[k]) > 0 for k in keys if k != "campos")
    if not mixed:   # a distortion-only loss: no colour gradient
        assert not np.any(grads["shs" if f["use_sh"] else "colors_precomp"])
        if f["pose"]:
            assert not np.any(grads["campos"])   # campos reaches only the SH colours
    cams = [k for k in keys if k in ("viewmatrix", "projmatrix", "campos")]
    check_grads(grads, ref, [k for k in keys if k not in cams], tag=f"dist:grad:{form}:{int(mixed)}")
    for k in cams:   # (the bar of the existing camera-gradient tests)
        assert np.linalg.norm(ref[k]) == 0 and not np.any(grads[k]) or rel_l2(grads[k], ref[k]) <= GRAD_RTOL_ALL, k


# ---- 2. shift invariance ----------------------------------------------------------------------------------------------------------
def test_a_depth_value_shifted_by_1000_gives_the_same_plane():
    """(depth values on a 2^-12 grid, so that d + 1000 is exact in float32 and the two planes differ by the kernel's rounding
    alone; without the per-pixel origin d·A − B is a difference of products near 1000 and the bar is missed)"""
    sc = _scene()
    z = torch.round(sc.means3D[:, 2] * 4096.0) / 4096.0
    assert torch.equal((z + 1000.0) - 1000.0, z)
    near, _ = _run(sc, _gq(), aux=z)
    far, _ = _run(sc, _gq(), aux=z + 1000.0)
    d = np.abs(far["distortion"].astype(np.float64) - near["distortion"])
    print(f"shift by 1000: max |Δ| {d.max():.3e} at a peak of {near['distortion'].max():.3f}")
    check_image(far["distortion"], near["distortion"], name="distortion shifted", tag="dist:shift")


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------------------
def _stacked(ops, zs):
    sc = make_scene(len(ops), 17, 17, sh_degree=0, seed=1315)   # (the optical axis meets the centre of pixel (8, 8))
    sc.means3D = torch.tensor([[0.0, 0.0, z] for z in zs])
    sc.opacities = torch.tensor(ops)[:, None]
    return sc.to(DEV)


def _plane(s, **extra):
    with torch.no_grad():
        return GaussianRasterizer(s.settings()._replace(return_distortion=True, **extra))(
            means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)[-1]


def test_closed_forms_on_the_gpu():
    one = _plane(_stacked([0.7], [3.0]))
    assert one.shape == (17, 17) and not bool(one.any())          # one Gaussian: exactly 0 everywhere
    a1, a2, d1, d2 = 0.5, 0.25, 2.0, 5.0
    two = _plane(_stacked([a1, a2], [d1, d2]))
    w1, w2 = a1, a2 * (1 - a1)
    assert abs(float(two[8, 8]) - 2 * w1 * w2 * (d2 - d1)) <= 1e-6
    assert float(two.max()) > 0 and float(two.min()) >= 0


# ---- 4. bit-reproducibility ---------------------------------------------------------------------------------------------------------
def test_plane_is_bit_identical_across_sorts_runs_and_forward_kinds():
    sc = _scene()
    base, _ = _run(sc, _gq())
    again, _ = _run(sc, _gq())
    assert np.array_equal(base["distortion"], again["distortion"])
    for sort in ("global", "global_3pass", "per_tile"):
        got, _ = _run(sc, _gq(), depth_sort=sort)
        assert np.array_equal(got["distortion"], base["distortion"]), sort
    infer = _plane(sc.to(DEV), sh_max_degree=3)
    assert np.array_equal(infer.cpu().numpy(), base["distortion"])


# ---- 5. launch sets ---------------------------------------------------------------------------------------------------------------
def test_launch_set_and_gaussian_sets_equal_per_view_calls():
    scs = [dr.clustered_scene(seed=1301 + b).to(DEV) for b in range(2)]
    gQ = torch.stack([_gq(1350 + v) for v in range(2)]).to(DEV)
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 2, dtype=torch.float32, device=DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3, return_distortion=True)
    leaf = lambda t: t.detach().clone().requires_grad_(True)

    def per_view(s, view, proj, cam, gs):
        m, o, c = leaf(s.means3D), leaf(s.opacities), leaf(s.cov3D)
        outs = []
        for v in range(len(gs)):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            q = GaussianRasterizer(r)(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=s.shs, cov3D_precomp=c)[-1]
            (q * gs[v]).sum().backward()
            outs.append(q.detach())
        return torch.stack(outs), m.grad, o.grad, c.grad

    # one Gaussian set, two views
    s = scs[0]
    view, proj, cam = _cams(s, 2)
    bg = s.bg.reshape(1, 3).expand(2, 3).contiguous()
    m, o, c = leaf(s.means3D), leaf(s.opacities), leaf(s.cov3D)
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=s.shs, cov3D_precomp=c)
    assert len(out) == 4 and out[-1].shape == (2, H, W)
    (out[-1] * gQ).sum().backward()
    ref = per_view(s, view, proj, cam, gQ)
    assert torch.equal(out[-1].detach(), ref[0])
    for a, b in zip((m.grad, o.grad, c.grad), ref[1:]):
        assert float(b.abs().max()) > 0 and rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL
    # two Gaussian sets of one view each
    cams = [_cams(s, 1) for s in scs]
    view, proj, cam = (torch.cat([c_[i] for c_ in cams]) for i in range(3))
    bg = torch.stack([s.bg for s in scs])
    stk = lambda f: leaf(torch.stack([f(s) for s in scs]))
    m, o, c = stk(lambda s: s.means3D), stk(lambda s: s.opacities), stk(lambda s: s.cov3D)
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=stk(lambda s: s.shs), cov3D_precomp=c)
    (out[-1] * gQ).sum().backward()
    assert m.grad.shape == (2, P, 3)
    for b in range(2):
        ref = per_view(scs[b], *cams[b], gQ[b:b + 1])
        assert torch.equal(out[-1][b:b + 1].detach(), ref[0])
        for a, r in zip((m.grad[b], o.grad[b], c.grad[b]), ref[1:]):
            assert rel_l2(a.cpu().numpy(), r.cpu().numpy()) <= GRAD_RTOL


# ---- 6. modes ---------------------------------------------------------------------------------------------------------------------
def test_scissor_inside_equal_outside_zero():
    sc = _scene()
    full, _ = _run(sc, _gq())
    win, _ = _run(sc, _gq(), scissor=(16, 0, 32, 16))
    assert np.array_equal(win["distortion"][0:16, 16:32], full["distortion"][0:16, 16:32])
    mask = np.ones((H, W), bool)
    mask[0:16, 16:32] = False
    assert not np.any(win["distortion"][mask]) and np.any(win["distortion"])


def test_antialiasing_matches_the_reference():
    sc = _scene()
    kw = dr.scene_inputs(sc, torch.float64, leaf=True)
    ref = dr.run_reference(sc, kw, antialiasing=True)
    (ref["distortion"] * _gq().double()).sum().backward()
    out, grads = _run(sc, _gq(), antialiasing=True)
    plain, _ = _run(sc, _gq())
    assert not np.array_equal(out["distortion"], plain["distortion"])
    check_image(out["distortion"], ref["distortion"].detach().numpy(), name="distortion (antialiasing)", tag="dist:aa")
    keys = ["means3D", "opacities", "cov3D_precomp"]
    for k in keys:
        print(f"antialiasing grad {k}: rel-L2 {rel_l2(grads[k], kw[k].grad.numpy()):.3e}")
    check_grads(grads, {k: kw[k].grad.numpy() for k in keys}, keys, tag="dist:grad:aa")


def test_a_missed_list_hint_changes_nothing():
    import ggrt_official_amd.rasterizer as R
    sc = _scene()
    R.clear_list_hints()
    first, g1 = _run(sc, _gq())                           # exact mode (first call of the shape)
    key = next(k for k in R._hints if k[1] == P)
    with R._hint_lock:
        R._hints[key] = [(64, 1)]                           # a guess far too small: the call repairs itself
    before = R.list_hint_stats()["missed"]
    again, g2 = _run(sc, _gq())
    assert R.list_hint_stats()["missed"] == before + 1
    assert np.array_equal(first["distortion"], again["distortion"]) and np.array_equal(first["color"], again["color"])
    for k in g1:
        assert rel_l2(g2[k], g1[k]) <= GRAD_RTOL, k
    R.clear_list_hints()


def test_sync_free_graph_replay_equals_eager():
    s = _scene().to(DEV)
    gQ = _gq().to(DEV)
    rs = s.settings()._replace(list_capacity=20_000, sh_max_degree=3, return_distortion=True)
    means, shs, op, cov = [t.clone().requires_grad_() for t in (s.means3D, s.shs, s.opacities, s.cov3D)]
    m2d = torch.zeros_like(means, requires_grad=True)
    rast = GaussianRasterizer(rs)

    def fwd_bwd():
        for t in (means, shs, op, cov, m2d):
            t.grad = None
        out = rast(means3D=means, means2D=m2d, opacities=op, shs=shs, cov3D_precomp=cov)
        (out[-1] * gQ).sum().backward()
        return out[-1]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_plane = fwd_bwd()
    g_grads = [means.grad, op.grad, cov.grad]
    with torch.no_grad():
        op.mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    got = [g_plane.detach().clone()] + [t.clone() for t in g_grads]
    e = [t.detach().clone().requires_grad_() for t in (means, shs, op, cov)]
    out = GaussianRasterizer(s.settings()._replace(sh_max_degree=3, return_distortion=True))(
        means3D=e[0], means2D=torch.zeros_like(e[0]), opacities=e[2], shs=e[1], cov3D_precomp=e[3])
    (out[-1] * gQ).sum().backward()
    assert torch.equal(got[0], out[-1].detach())
    for a, b in zip(got[1:], [e[0].grad, e[2].grad, e[3].grad]):
        assert float(b.abs().max()) > 0 and rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL


def test_a_second_backward_over_one_forward():
    s = _scene().to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    m, o, c = leaf(s.means3D), leaf(s.opacities), leaf(s.cov3D)
    out = GaussianRasterizer(s.settings()._replace(sh_max_degree=3, return_distortion=True))(
        means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=s.shs, cov3D_precomp=c)
    loss = (out[-1] * _gq().to(DEV)).sum()
    g1 = torch.autograd.grad(loss, (m, o, c), retain_graph=True)
    g2 = torch.autograd.grad(loss, (m, o, c))
    for a, b in zip(g1, g2):
        assert float(a.abs().max()) > 0 and rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= GRAD_RTOL


# ---- 7. combined passes -------------------------------------------------------------------------------------------------------------
def test_features_and_distortion_in_one_backward_equal_two_backwards():
    sc = _scene()
    ex = _extras()
    feats, gF = ex["feats"], ex["gF"]
    both, g_both = _run(sc, _gq(), feats=feats, gF=gF)
    _, g_feat = _run(sc, torch.zeros(H, W), feats=feats, gF=gF)
    _, g_dist = _run(sc, _gq(), feats=feats, gF=torch.zeros_like(gF))
    assert both["features"].shape == (K, H, W)
    for k in ("means3D", "opacities", "cov3D_precomp", "features"):
        want = g_feat[k] + g_dist[k]
        assert np.abs(g_feat[k]).max() > 0 and (k == "features" or np.abs(g_dist[k]).max() > 0), k
        assert rel_l2(g_both[k], want) <= GRAD_RTOL, (k, rel_l2(g_both[k], want))


# ---- 8. off = the parent --------------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_distortion_call(monkeypatch):
    lib = _lib.load()
    sc = _scene()
    ex = _extras()
    col_only = dict(ex, gD=torch.zeros(H, W), gA=torch.zeros(H, W), gF=torch.zeros(K, H, W))
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_distortion_forward", lambda *a: calls.append("f") or 99)
        mp.setattr(lib, "ggr_distortion_backward", lambda *a: calls.append("b") or 99)
        off, g_off = _run(sc, None, col_only, distortion=False)
    assert "distortion" not in off and len(off) == 5 and not calls
    on, g_on = _run(sc, _gq(), col_only)
    assert len(on) == 6
    for k in off:
        assert np.array_equal(off[k], on[k]), k
    # with a distortion gradient of zero the other gradients are what they were
    zero, g_zero = _run(sc, torch.zeros(H, W), col_only)
    for k in g_off:
        assert rel_l2(g_zero[k], g_off[k]) <= GRAD_RTOL, k
    assert any(rel_l2(g_on[k], g_off[k]) > 1e-3 for k in ("means3D", "opacities"))
