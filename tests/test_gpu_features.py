"""The feature pass on the GPU (`-m gpu`): `features_precomp` / ggr_features_forward / ggr_features_backward.

K per-Gaussian channels composited in one pass over a forward's lists.  Checked: bit-exact identities with the colour and the
depth plane, K = 1, 4, 7, 16, 32 against the ⌈K/3⌉-call loop of the existing path (forward bit for bit, every gradient by
rel-L2 over all rows to helpers.GRAD_RTOL), the composed torch reference (tests/features_reference.py), camera gradients,
launch sets, every mode's contract, "off = as before", and the decoder.

"Bit-identical" is said of images.  Gradients of two runs are compared within rounding: they are accumulated with float
atomics in varying order."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views
from ggrt_official_amd.synthetic import make_scene, upstream_gradient
from tests.features_reference import rasterize_features
from tests.helpers import GRAD_RTOL, check_grads, check_image, rel_l2
from tests.test_gpu_alpha import CASES, _cams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _feats(P, K, seed, scale=1.0):
    return (torch.rand(P, K, generator=torch.Generator().manual_seed(seed)) * 2.0 - 0.5) * scale


def _fgrad(K, W, H, seed):
    """[K,H,W] upstream gradient of the feature planes, the scale of a colour channel's"""
    return torch.cat([upstream_gradient(W, H, seed=seed + i) for i in range((K + 2) // 3)])[:K].contiguous()


def _leaves(s, use_sh, use_cov, colors):
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    means, op = leaf(s.means3D), leaf(s.opacities)
    kw, leaves = {}, dict(means3D=means, opacities=op)
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(colors)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(s.scales)
        leaves["rotations"] = kw["rotations"] = leaf(s.rotations)
    return means, op, kw, leaves


def _run(sc, feats, gF, dL=None, use_sh=True, use_cov=True, colors=None, pose=False, **extra):
    """Forward + backward of Σ gF·features + Σ dL·colour on cuda:0 → (outputs as numpy, grads)."""
    s = sc.to(DEV)
    means, op, kw, leaves = _leaves(s, use_sh, use_cov, colors)
    m2d = torch.zeros_like(means, requires_grad=True)
    rs = s.settings()._replace(sh_max_degree=3, **extra)
    if pose:
        leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
        view, proj, cam = leaf(s.viewmatrix), leaf(s.projmatrix), leaf(s.campos)
        rs = rs._replace(viewmatrix=view, projmatrix=proj, campos=cam)
        leaves.update(viewmatrix=view, projmatrix=proj, campos=cam)
    if feats is not None:
        leaves["features"] = kw["features_precomp"] = feats.detach().clone().to(DEV).requires_grad_(True)
    out = GaussianRasterizer(rs)(means3D=means, means2D=m2d, opacities=op, **kw)
    loss = 0.0
    if dL is not None:
        loss = loss + (out[0] * dL.to(DEV)).sum()
    if gF is not None:
        loss = loss + (out[-1] * gF.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}
    return [o.detach().cpu().numpy() for o in out], grads


def _loop(sc, feats, gF, use_sh=True, use_cov=True, **extra):
    """The parent's only route: ⌈K/3⌉ calls of the existing path with `colors_precomp` set to 3-channel slices, bg = 0;
    returns (planes [K,H,W], gradients summed over the calls, dL/dfeatures)."""
    P, K = feats.shape
    sc0 = sc.to("cpu")
    sc0.bg = torch.zeros(3)
    planes, total, dfeat = [], None, np.zeros((P, K), np.float32)
    for k0 in range(0, K, 3):
        n = min(3, K - k0)
        sl = torch.zeros(P, 3)
        sl[:, :n] = feats[:, k0:k0 + n]
        dl = torch.zeros(3, sc.height, sc.width)
        dl[:n] = gF[k0:k0 + n]
        s = sc0.to(DEV)
        means, op, kw, leaves = _leaves(s, False, use_cov, sl)
        rs = s.settings()._replace(sh_max_degree=3, **extra)
        col = GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means, requires_grad=True), opacities=op, **kw)[0]
        (col * dl.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        planes.append(col.detach().cpu().numpy()[:n])
        g = {k: v.grad.detach().cpu().numpy() for k, v in leaves.items()}
        dfeat[:, k0:k0 + n] = g.pop("colors_precomp")[:, :n]
        total = g if total is None else {k: total[k] + g[k] for k in g}
    return np.concatenate(planes), total, dfeat


# ---- (a) bit-exact identities ------------------------------------------------------------------------------------------
def test_channels_equal_the_colour_and_the_depth_plane_bit_for_bit():
    P, W, H = 30000, 208, 160
    sc = make_scene(P, W, H, sh_degree=0, seed=611)
    sc.bg = torch.zeros(3)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(612))
    aux = torch.rand(P, generator=torch.Generator().manual_seed(613)) * 5.0
    feats = torch.cat([colors, aux[:, None], colors[:, :1]], dim=1)   # K = 5
    s = sc.to(DEV)
    with torch.no_grad():
        out = GaussianRasterizer(s.settings())(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                               colors_precomp=colors.to(DEV), cov3D_precomp=s.cov3D, aux_precomp=aux.to(DEV),
                                               features_precomp=feats.to(DEV))
    assert len(out) == 4 and out[3].shape == (5, H, W)
    color, depth, f = out[0], out[2], out[3]
    assert float(color.max()) > 0.3
    assert torch.equal(f[:3], color) and torch.equal(f[3], depth) and torch.equal(f[4], color[0])


# ---- (b) K channels against the loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 7, 16, 32])
def test_k_channels_equal_the_loop_of_three_channel_calls(K):
    P, W, H, D, use_sh, use_cov, aa, _, seed = CASES[K % len(CASES)]
    sc = make_scene(P, W, H, sh_degree=D, seed=seed)
    feats, gF = _feats(P, K, seed + 7), _fgrad(K, W, H, seed + 70)
    out, grads = _run(sc, feats, gF, dL=None, use_sh=False, use_cov=use_cov, colors=torch.zeros(P, 3), antialiasing=aa)
    planes, ref, dfeat = _loop(sc, feats, gF, use_cov=use_cov, antialiasing=aa)
    assert np.array_equal(out[-1], planes)
    for k, r in ref.items():
        e = rel_l2(grads[k], r)
        print(f"K={K} grad {k}: rel-L2 {e:.3e}")
        assert e <= GRAD_RTOL, f"K={K} grad {k}: rel-L2 {e:.3e}"
    e = rel_l2(grads["features"], dfeat)
    print(f"K={K} grad features: rel-L2 {e:.3e}")
    assert e <= GRAD_RTOL, f"K={K} dL/dfeatures: rel-L2 {e:.3e}"
    assert not np.any(grads["colors_precomp"])   # a features-only loss: no colour gradient


# ---- (c) against the composed torch reference ---------------------------------------------------------------------------
REF_CASES = [(c, K, fonly, mag) for c, K, fonly, mag in zip(CASES, (4, 7, 5, 3), (False, False, True, False), (1.0, 1.0, 1.0, 10.0))]


@pytest.mark.parametrize("case,K,features_only,magnitude", REF_CASES)
def test_image_and_gradients_match_the_composed_torch_reference(case, K, features_only, magnitude):
    P, W, H, D, use_sh, use_cov, aa, _, seed = case
    sc = make_scene(P, W, H, sh_degree=D, seed=seed)
    feats, gF = _feats(P, K, seed + 9, magnitude), _fgrad(K, W, H, seed + 90)
    dL = None if features_only else upstream_gradient(W, H, seed=seed + 50)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    leaf = lambda t: t.float().clone().requires_grad_(True)
    m, op, f = leaf(sc.means3D), leaf(sc.opacities), leaf(feats)
    kw = dict(cov3D_precomp=leaf(sc.cov3D)) if use_cov else dict(scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    kw.update(dict(shs=leaf(sc.shs)) if use_sh else dict(colors_precomp=leaf(colors)))
    color, radii, _, planes = rasterize_features(m, op, f, sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg, W, H, sc.tanfovx,
                                                 sc.tanfovy, D, sh_cap=3, antialiasing=aa, **kw)
    ((planes * gF).sum() + ((color * dL).sum() if dL is not None else 0.0)).backward()
    ref = dict(means3D=m.grad, opacities=op.grad, features=f.grad, **{k: v.grad for k, v in kw.items()})
    out, grads = _run(sc, feats, gF, dL, use_sh=use_sh, use_cov=use_cov, colors=colors, antialiasing=aa, return_alpha=True)
    assert len(out) == 5 and np.array_equal(out[1], radii.numpy())
    check_image(out[0], color.detach().numpy(), tag=f"feat:color{seed}")
    check_image(out[-1], planes.detach().numpy(), name="features", tag=f"feat:planes{seed}")
    if magnitude != 1.0:
        assert rel_l2(out[-1], planes.detach().numpy()) <= 1e-5
    keys = [k for k in ref if not (features_only and k in ("shs", "colors_precomp"))]
    if features_only:
        assert not np.any(grads["shs" if use_sh else "colors_precomp"])
    check_grads(grads, {k: ref[k].numpy() for k in keys}, keys, tag=f"feat:grad{seed}")


# ---- (d) camera gradients under a features-only loss ------------------------------------------------------------------
def test_camera_gradients_under_a_features_only_loss():
    W, H, P, K = 160, 128, 12000, 4
    sc = make_scene(P, W, H, sh_degree=3, seed=631)
    feats, gF = _feats(P, K, 632), _fgrad(K, W, H, 633)
    leaf = lambda t: t.float().clone().requires_grad_(True)
    view, proj, cam = leaf(sc.viewmatrix), leaf(sc.projmatrix), leaf(sc.campos)
    planes = rasterize_features(sc.means3D, sc.opacities, feats, view, proj, cam, sc.bg, W, H, sc.tanfovx, sc.tanfovy, 3,
                                shs=sc.shs, cov3D_precomp=sc.cov3D, sh_cap=3)[3]
    (planes * gF).sum().backward()
    _, grads = _run(sc, feats, gF, None, pose=True)
    for k, r in (("viewmatrix", view.grad), ("projmatrix", proj.grad)):
        e = rel_l2(grads[k], r.numpy())
        assert e <= 1e-3, (k, e)     # (the bar of the existing camera-gradient tests: helpers.GRAD_RTOL_ALL)
    assert not np.any(grads["campos"])   # campos reaches only the SH colours


# ---- (e) launch sets ---------------------------------------------------------------------------------------------------
def test_launch_set_and_gaussian_sets_equal_per_view_calls():
    K = 6
    scs = [make_scene(8000, 160, 128, sh_degree=3, seed=640 + b).to(DEV) for b in range(2)]
    feats = [_feats(8000, K, 650 + b).to(DEV) for b in range(2)]
    gF = torch.stack([_fgrad(K, 160, 128, 660 + 3 * v) for v in range(4)]).to(DEV)
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 4, dtype=torch.float32, device=DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3)
    leaf = lambda t: t.detach().clone().requires_grad_(True)

    def per_view(s, f, view, proj, cam, gs):
        m, o, ff = leaf(s.means3D), leaf(s.opacities), leaf(f)
        outs = []
        for v in range(len(gs)):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            p = GaussianRasterizer(r)(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=s.shs, cov3D_precomp=s.cov3D,
                                      features_precomp=ff)[-1]
            (p * gs[v]).sum().backward()
            outs.append(p.detach())
        return torch.stack(outs), m.grad, o.grad, ff.grad

    # one Gaussian set, four views
    s = scs[0]
    view, proj, cam = _cams(s, 4)
    bg = s.bg.reshape(1, 3).expand(4, 3).contiguous()
    m, o, ff = leaf(s.means3D), leaf(s.opacities), leaf(feats[0])
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=s.shs, cov3D_precomp=s.cov3D, features_precomp=ff)
    assert len(out) == 4 and out[-1].shape == (4, K, 128, 160)
    (out[-1] * gF).sum().backward()
    ref = per_view(s, feats[0], view, proj, cam, gF)
    assert torch.equal(out[-1].detach(), ref[0])
    for a, b in zip((m.grad, o.grad, ff.grad), ref[1:]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL
    # two Gaussian sets of two views each
    cams = [_cams(s, 2) for s in scs]
    view, proj, cam = (torch.cat([c[i] for c in cams]) for i in range(3))
    bg = torch.stack([scs[v // 2].bg for v in range(4)])
    stk = lambda f: leaf(torch.stack([f(s) for s in scs]))
    m, o, ff = stk(lambda s: s.means3D), stk(lambda s: s.opacities), leaf(torch.stack(feats))
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=stk(lambda s: s.shs), cov3D_precomp=stk(lambda s: s.cov3D),
                          features_precomp=ff)
    (out[-1] * gF).sum().backward()
    assert ff.grad.shape == (2, 8000, K)
    for b in range(2):
        ref = per_view(scs[b], feats[b], *cams[b], gF[2 * b:2 * b + 2])
        assert torch.equal(out[-1][2 * b:2 * b + 2].detach(), ref[0])
        for a, r in zip((m.grad[b], o.grad[b], ff.grad[b]), ref[1:]):
            assert rel_l2(a.cpu().numpy(), r.cpu().numpy()) <= GRAD_RTOL


# ---- (f) modes ---------------------------------------------------------------------------------------------------------
def _small(seed, K=5):
    sc = make_scene(20000, 176, 144, sh_degree=3, seed=seed)
    return sc, _feats(20000, K, seed + 1), _fgrad(K, 176, 144, seed + 2)


def test_scissor_inside_equal_outside_zero():
    sc, feats, gF = _small(671)
    full, _ = _run(sc, feats, gF)
    win, _ = _run(sc, feats, gF, scissor=(32, 48, 112, 96))
    assert np.array_equal(win[-1][:, 48:96, 32:112], full[-1][:, 48:96, 32:112])
    mask = np.ones((144, 176), bool)
    mask[48:96, 32:112] = False
    assert not np.any(win[-1][:, mask])


def test_inference_equals_the_training_forward():
    sc, feats, gF = _small(672)
    train, _ = _run(sc, feats, gF)
    s = sc.to(DEV)
    with torch.no_grad():
        out = GaussianRasterizer(s.settings()._replace(sh_max_degree=3))(
            means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D,
            features_precomp=feats.to(DEV))
    assert np.array_equal(out[-1].cpu().numpy(), train[-1]) and np.array_equal(out[0].cpu().numpy(), train[0])


def test_a_missed_list_hint_changes_nothing():
    import ggrt_official_amd.rasterizer as R
    sc, feats, gF = _small(673)
    R.clear_list_hints()
    first, g1 = _run(sc, feats, gF)                       # exact mode (first call of the shape)
    key = next(k for k in R._hints if k[1] == 20000)
    with R._hint_lock:
        R._hints[key] = [(64, 1)]                           # a guess far too small: the call repairs itself
    before = R.list_hint_stats()["missed"]
    again, g2 = _run(sc, feats, gF)
    assert R.list_hint_stats()["missed"] == before + 1
    assert np.array_equal(first[-1], again[-1]) and np.array_equal(first[0], again[0])
    for k in g1:
        assert rel_l2(g2[k], g1[k]) <= GRAD_RTOL, k
    R.clear_list_hints()


def test_sync_free_graph_replay_equals_eager():
    sc, feats, gF = _small(674)
    s = sc.to(DEV)
    gF, f0 = gF.to(DEV), feats.to(DEV)
    rs = s.settings()._replace(list_capacity=400_000, sh_max_degree=3)
    means, shs, op, cov, ff = [t.clone().requires_grad_() for t in (s.means3D, s.shs, s.opacities, s.cov3D, f0)]
    m2d = torch.zeros_like(means, requires_grad=True)
    rast = GaussianRasterizer(rs)

    def fwd_bwd():
        for t in (means, shs, op, cov, m2d, ff):
            t.grad = None
        out = rast(means3D=means, means2D=m2d, opacities=op, shs=shs, cov3D_precomp=cov, features_precomp=ff)
        (out[-1] * gF).sum().backward()
        return out[-1]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_planes = fwd_bwd()
    g_grads = [means.grad, op.grad, cov.grad, ff.grad]
    with torch.no_grad():
        op.mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    got = [g_planes.detach().clone()] + [t.clone() for t in g_grads]
    e = [t.detach().clone().requires_grad_() for t in (means, shs, op, cov, ff)]
    out = GaussianRasterizer(s.settings()._replace(sh_max_degree=3))(
        means3D=e[0], means2D=torch.zeros_like(e[0]), opacities=e[2], shs=e[1], cov3D_precomp=e[3], features_precomp=e[4])
    (out[-1] * gF).sum().backward()
    assert torch.equal(got[0], out[-1].detach())
    for a, b in zip(got[1:], [e[0].grad, e[2].grad, e[3].grad, e[4].grad]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL


def test_a_second_backward_over_one_forward():
    sc, feats, gF = _small(675)
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    m, o, ff = leaf(s.means3D), leaf(s.opacities), leaf(feats)
    out = GaussianRasterizer(s.settings()._replace(sh_max_degree=3))(
        means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=s.shs, cov3D_precomp=s.cov3D, features_precomp=ff)
    loss = (out[-1] * gF.to(DEV)).sum()
    g1 = torch.autograd.grad(loss, (m, o, ff), retain_graph=True)
    g2 = torch.autograd.grad(loss, (m, o, ff))
    for a, b in zip(g1, g2):
        assert float(a.abs().max()) > 0 and rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= GRAD_RTOL


# ---- (g) off = the parent ----------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_feature_call(monkeypatch):
    lib = _lib.load()
    sc, feats, gF = _small(681)
    dL = upstream_gradient(176, 144, seed=682)
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_features_forward", lambda *a: calls.append("f") or 99)
        mp.setattr(lib, "ggr_features_backward", lambda *a: calls.append("b") or 99)
        off, g_off = _run(sc, None, None, dL)
    assert len(off) == 3 and not calls
    on, g_on = _run(sc, feats, gF, dL)
    assert len(on) == 4
    for a, b in zip(off, on[:3]):
        assert np.array_equal(a, b)
    # with a features gradient of zero the colour's gradients are what they were
    zero, g_zero = _run(sc, feats, torch.zeros_like(gF), dL)
    for k in g_off:
        assert rel_l2(g_zero[k], g_off[k]) <= GRAD_RTOL, k
    assert not np.any(g_zero["features"]) and np.any(g_on["features"])


# ---- (h) the decoder ---------------------------------------------------------------------------------------------------
def test_decoder_features_equal_per_view_rasterizer_calls():
    from ggrt_official_amd import splatting as S
    gen = torch.Generator().manual_seed(691)
    b, v, n, d_sh, h, w, K = 2, 3, 4000, 16, 96, 128, 5
    ext = torch.eye(4).repeat(b, v, 1, 1)
    ext[..., 0, 3] = torch.linspace(-0.2, 0.2, v)
    Kmat = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    means = torch.randn(b, n, 3, generator=gen) * torch.tensor([0.6, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(b, n, 3, 3, generator=gen) * 0.05
    cov = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3)
    harm = torch.randn(b, n, 3, d_sh, generator=gen) * 0.3
    opac = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    feats = torch.randn(b, n, K, generator=gen)
    to = lambda t: t.to(DEV)
    gs = S.Gaussians(to(means), to(cov), to(harm), to(opac))
    args = (gs, to(ext), to(Kmat), to(near), to(far), (h, w))
    dec = S.DecoderSplattingCUDA(sh_max_degree=4).to(DEV)
    with torch.no_grad():
        plain = dec(*args, depth_mode="depth")
        out = dec(*args, depth_mode="depth", gaussian_features=to(feats))
        assert plain.features is None and out.features.shape == (b, v, K, h, w)
        assert torch.equal(out.color, plain.color) and torch.equal(out.depth, plain.depth)
        # the same views one rasterizer call each (the fused call site with batched=False): the launch set's planes, bit for bit
        flat = lambda t: t.flatten(0, 1)
        bg = torch.zeros(b * v, 3, device=DEV)
        per_view = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w), bg, gs,
                                        [n_ // v for n_ in range(b * v)], "depth", batched=False, sh_max_degree=4,
                                        gaussian_features=to(feats))
        assert len(per_view) == 3
        assert torch.equal(per_view[-1].reshape(b, v, K, h, w), out.features)
        assert torch.equal(per_view[0].reshape(b, v, 3, h, w), out.color)
        # the reference-shaped call site (torch pre-processing, one call per view) takes the keyword too, with and without a
        # depth pass
        slow = S.DecoderSplattingCUDA(sh_max_degree=4, fused_inputs=False).to(DEV)
        o2 = slow(*args, depth_mode="depth", gaussian_features=to(feats))
        o3 = slow(*args, gaussian_features=to(feats))
        assert o2.features.shape == out.features.shape and torch.equal(o3.features, o2.features)
        assert float((o2.features - out.features).abs().mean()) < 1e-5 * max(1.0, float(out.features.abs().max()))
    leaf = to(feats).clone().requires_grad_(True)
    o = dec(*args, gaussian_features=leaf)
    o.features.sum().backward()
    assert leaf.grad.shape == feats.shape and float(leaf.grad.abs().max()) > 0
