"""The hit pass's backward on the GPU (`-m gpu`): `hits_grad` / ggr_pixel_hits_backward.

With `hits_grad=True` the `weight` and `rest` of a `PixelHits` are differentiable: a loss over them reaches means, opacities,
covariances / scales / rotations and the camera.  Checked: the float64 torch reference on the frozen oracle's lists
(tests/hits_grad_reference.py) at K = 1, 8 and 32, the alpha backward and the feature backward as independent HIP witnesses, the
padding contract, a missing gradient, composition with the other passes in one scratch, launch sets, the scissor, antialiasing,
a missed list hint, the sync-free mode under graph capture, a second backward, the forms of the depth sort and "off = as before".

Scenes: hits_reference.REF_CASES (multi-batch lists and early stops; an odd 83×45 frame with partial tiles, scales + rotations,
antialiasing; small Gaussians whose pixels mostly leave slots unfilled).  tests/test_hits_grad_reference.py fixes on the CPU that
the float32 and the float64 reference agree on every index and count at every K used here, so the GPU is held to equality in
EVERY pixel before any gradient is compared.

Bars.  Gradients against the reference: helpers.check_grads as it is (rel-L2 ≤ 1e-3 over all rows, ≤ GRAD_RTOL = 2e-5 once the
flip rule's rows are set aside), the camera tensors at GRAD_RTOL_ALL like the existing camera-gradient tests.  Two HIP runs that
sum the SAME per-(pixel, entry) terms are compared within GRAD_RTOL: the sums are accumulated with float atomics, whose order
varies — except in the padding test, which asks for bit equality where the sums do not depend on that order (a loss confined to
quadrants that share no Gaussian more than twice) and for GRAD_RTOL on the whole frame."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import GaussianRasterizer, PixelHits, _lib, composite_hits, rasterize_views
from ggrt_official_amd.synthetic import upstream_gradient
from tests import hits_grad_reference as hg
from tests.helpers import GRAD_RTOL, GRAD_RTOL_ALL, check_grads, rel_l2
from tests.test_gpu_alpha import _cams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, B, Cs = list(hg.REF_CASES)   # A_sh_cov, B_colours_scale_rot_aa_odd_frame, C_small_gaussians_unfilled_slots
GEOM = {True: ["means3D", "opacities", "cov3D_precomp"], False: ["means3D", "opacities", "scales", "rotations"]}
CAMS = ["viewmatrix", "projmatrix", "campos"]


def _g(name, K, seed=2101):
    """fixed upstream gradients of mixed sign: (G [K,H,W], Gr [H,W])"""
    _P, W, H = hg.REF_CASES[name][:3]
    gen = torch.Generator().manual_seed(seed + K)
    return torch.randn(K, H, W, generator=gen) / (H * W), torch.randn(H, W, generator=gen) / (H * W)


def _leaves(name, pose=False):
    """(scene on the device, rasterizer keyword inputs, leaves by name) of a reference scene in its own input form"""
    _P, _W, _H, _D, use_sh, use_cov, _aa, _seed = hg.REF_CASES[name]
    sc, colors = hg.ref_scene(name)
    s = sc.to(DEV)
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    leaves = dict(means3D=leaf(s.means3D), opacities=leaf(s.opacities))
    kw = dict(means3D=leaves["means3D"], opacities=leaves["opacities"])
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(colors)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"], leaves["rotations"] = kw["scales"], kw["rotations"] = leaf(s.scales), leaf(s.rotations)
    if pose:
        leaves.update(viewmatrix=leaf(s.viewmatrix), projmatrix=leaf(s.projmatrix), campos=leaf(s.campos))
    return s, kw, leaves


def _settings(name, s, leaves, K, **settings):
    aa = settings.pop("antialiasing", hg.REF_CASES[name][6])
    rs = s.settings()._replace(sh_max_degree=3, return_hits=K, antialiasing=aa, **settings)
    if "viewmatrix" in leaves:
        rs = rs._replace(viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"], campos=leaves["campos"])
    return rs


def _forward(name, K, pose=False, features=None, **settings):
    s, kw, leaves = _leaves(name, pose)
    settings.setdefault("hits_grad", True)
    rs = _settings(name, s, leaves, K, **settings)
    if features is not None:
        leaves["features"] = kw["features_precomp"] = features.detach().clone().to(DEV).requires_grad_(True)
    out = GaussianRasterizer(rs)(means2D=torch.zeros_like(leaves["means3D"], requires_grad=True), **kw)
    assert K == 0 or isinstance(out[-1], PixelHits)
    return out, leaves


def _np_grads(leaves):
    torch.cuda.synchronize()
    return {k: (np.zeros(tuple(v.shape), np.float32) if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}


def _run(name, K, gw, gr, pose=False, more=None, **settings):
    """forward + backward of Σ gw·weight + Σ gr·rest (a None term is left out; `more(out)` adds to the loss) → (hits, grads)"""
    out, leaves = _forward(name, K, pose, **settings)
    h = out[-1]
    loss = 0.0
    if gw is not None:
        loss = loss + (h.weight * gw.to(DEV)).sum()
    if gr is not None:
        loss = loss + (h.rest * gr.to(DEV)).sum()
    if more is not None:
        loss = loss + more(out)
    loss.backward()
    return h, _np_grads(leaves)


def _close(a, b, keys, tag, rtol=GRAD_RTOL):
    for k in keys:
        r = rel_l2(a[k], b[k])
        print(f"{tag} {k}: rel-L2 {r:.3e}, |ref| {np.linalg.norm(b[k]):.3e}")
        assert np.linalg.norm(b[k]) > 0 and r <= rtol, (tag, k, r)


# ---- 1. against the float64 reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [(A, 8), (B, 8), (Cs, 8), (A, 1), (B, 1), (Cs, 1), (Cs, 32)])
def test_gradients_match_the_float64_reference(name, K):
    use_cov = hg.REF_CASES[name][5]
    G, Gr = _g(name, K)
    _kw, ref = hg.ref_hits(name, K)
    h, grads = _run(name, K, G, Gr, pose=True)
    assert h.weight.requires_grad and h.rest.requires_grad and not h.index.requires_grad and not h.count.requires_grad
    differing = (h.index.cpu().to(torch.int64) != ref["index"]).any(0) | (h.count.cpu().to(torch.int64) != ref["count"])
    print(f"{name} K={K}: {int(differing.sum())} pixels differ from the reference in an index or the count; "
          f"{int((ref['count'] > K).sum())} pixels with a rest, {int((ref['count'] < K).sum())} with unfilled slots")
    assert not bool(differing.any())
    want = hg.ref_grads(name, K, G, Gr)
    keys = GEOM[use_cov]
    for k in keys + CAMS:
        print(f"{name} K={K} grad {k}: rel-L2 {rel_l2(grads[k], want[k]):.3e}, |ref| {np.linalg.norm(want[k]):.3e}")
    assert all(np.linalg.norm(want[k]) > 0 for k in keys + CAMS[:2])
    colour = "shs" if "shs" in grads else "colors_precomp"
    assert not np.any(grads[colour]) and not np.any(grads["campos"]) and not np.any(want["campos"])   # the weights see no colour
    check_grads(grads, want, keys, tag=f"hitsgrad:{name}:{K}")
    for k in CAMS[:2]:   # (the bar of the existing camera-gradient tests)
        assert rel_l2(grads[k], want[k]) <= GRAD_RTOL_ALL, k


# ---- 2. the alpha backward as a witness --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [(A, 8), (Cs, 1)])
def test_unit_gradients_equal_the_alpha_backward(name, K):
    """G ≡ 1 and Gr ≡ 1: the loss is Σ_k weight + rest = alpha summed over the frame"""
    _P, W, H = hg.REF_CASES[name][:3]
    _h, grads = _run(name, K, torch.ones(K, H, W), torch.ones(H, W))
    s, kw, leaves = _leaves(name)
    out = GaussianRasterizer(_settings(name, s, leaves, 0, return_alpha=True))(means2D=torch.zeros_like(leaves["means3D"]), **kw)
    out[3].sum().backward()
    _close(grads, _np_grads(leaves), GEOM[hg.REF_CASES[name][5]], f"alpha witness {name} K={K}")


# ---- 3. the feature backward as a witness ------------------------------------------------------------------------------------------
def test_composite_over_unfilled_pixels_equals_the_feature_pass():
    name, K = Cs, 8
    P, W, H = hg.REF_CASES[name][:3]
    D = torch.randn(H, W, generator=torch.Generator().manual_seed(2111)).to(DEV) / (H * W)
    values = torch.rand(P, generator=torch.Generator().manual_seed(2112)) * 2.0 - 0.5
    # the hit route: composite_hits over differentiable weights
    out, lh = _forward(name, K)
    lh["values"] = values.clone().to(DEV).requires_grad_(True)
    m = (out[-1].count <= K).float()
    assert 0.5 < float(m.mean()) and bool((out[-1].count > 0).any())
    comp = composite_hits(lh["values"], out[-1])
    (m * D * comp).sum().backward()
    g_hits = _np_grads(lh)
    # the feature route: the same values as one feature channel
    out, lf = _forward(name, 0, features=values[:, None], hits_grad=False)
    assert torch.allclose(out[-1][0] * m, comp.detach() * m, rtol=1e-5, atol=1e-6)
    (m * D * out[-1][0]).sum().backward()
    g_feat = _np_grads(lf)
    _close(g_hits, g_feat, GEOM[True], "feature witness")
    r = rel_l2(g_hits["values"], g_feat["features"][:, 0])
    print(f"feature witness dL/dvalues: rel-L2 {r:.3e}")
    assert r <= GRAD_RTOL


# ---- 4. padding is never read ------------------------------------------------------------------------------------------------------
def _order_free_quadrants(name):
    """[H,W] bool: a union of 8×8 quadrants (one wave each) chosen so that no Gaussian is composited in more than TWO of them.
    A wave commits one atomic per (Gaussian, record slot); a record slot that starts at zero and receives at most two addends
    holds a + b whatever their order (float addition is commutative; it is not associative), and preprocess_bwd has no atomic
    (the camera sums apart, which are not compared).  The gradients of a loss confined to these quadrants are therefore
    bit-reproducible from run to run — the only setting in which "bit for bit" can be asked of two backwards here."""
    P, W, H = hg.REF_CASES[name][:3]
    with torch.no_grad():
        out, _leaves_ = _forward(name, 32, hits_grad=False)
    assert int(out[-1].count.max()) <= 32, "the index slots must list every composited entry"
    idx, cnt = out[-1].index.cpu().numpy(), out[-1].count.cpu().numpy()
    used, mask = np.zeros(P, np.int64), torch.zeros(H, W, dtype=torch.bool)
    quads = [(qy, qx) for qy in range(0, H, 8) for qx in range(0, W, 8)]
    quads.sort(key=lambda q: -int(cnt[q[0]:q[0] + 8, q[1]:q[1] + 8].max()))   # (the busiest first: they hold the pixels with a rest)
    for qy, qx in quads:
        ids = np.unique(idx[:, qy:qy + 8, qx:qx + 8])
        ids = ids[ids >= 0]
        if ids.size and bool((used[ids] < 2).all()):
            used[ids] += 1
            mask[qy:qy + 8, qx:qx + 8] = True
    return mask


@pytest.mark.parametrize("name,K", [(Cs, 8), (Cs, 32)])
def test_nan_in_the_padding_reaches_no_result(name, K):
    """Upstream gradients that hold NaN at every slot k >= count and at `rest` where count <= K — in EVERY pixel of the frame:
    every result is finite and equals, bit for bit, the run with zeros there.

    Two backwards are comparable bit for bit only where their sums do not depend on the order of the float atomics (two
    IDENTICAL full-frame runs differ in the last bits: measured max |Δ| 4.7e-10 means3D, 2.9e-11 opacities, 1.8e-7 cov3D_precomp,
    rel-L2 below 4e-8).  So the test runs two losses.  (a) Gradients on the whole frame: finite, and equal to the zero-filled
    run within GRAD_RTOL.  (b) The same gradients confined to `_order_free_quadrants` — zero elsewhere, the NaN still in every
    padded place of the frame: finite and BIT FOR BIT equal to the zero-filled run."""
    _P, W, H = hg.REF_CASES[name][:3]
    G, Gr = _g(name, K)
    keys = GEOM[hg.REF_CASES[name][5]]
    quads = _order_free_quadrants(name)
    print(f"{name} K={K}: {int(quads.sum())} of {H * W} pixels in the order-free quadrants")
    assert int(quads.sum()) >= 8 * 64
    res = {}
    for part, keep in (("frame", torch.ones(H, W, dtype=torch.bool)), ("quadrants", quads)):
        for fill in (0.0, float("nan")):
            out, leaves = _forward(name, K)
            h = out[-1]
            slot = torch.arange(K, device=DEV)[:, None, None]
            pad_w, pad_r = slot >= h.count[None], h.count <= K
            k_dev = keep.to(DEV)
            # the kept pixels meet every case: unfilled slots, a padded rest, and (K = 8) a rest that is in use
            assert bool((pad_w & k_dev).any()) and bool((pad_r & k_dev).any()) and (K == 32 or bool((~pad_r & k_dev).any()))
            assert bool(((h.count > 0) & k_dev).sum() >= 100)
            gw = torch.where(pad_w, torch.full((), fill, device=DEV), (G * keep).to(DEV))
            gr = torch.where(pad_r, torch.full((), fill, device=DEV), (Gr * keep).to(DEV))
            assert fill == 0.0 or (bool(torch.isnan(gw[pad_w]).all()) and bool(torch.isnan(gr[pad_r]).all()))
            got = torch.autograd.grad([h.weight, h.rest], [leaves[k] for k in keys], [gw, gr])
            torch.cuda.synchronize()
            res[part, fill != 0.0] = {k: t.cpu() for k, t in zip(keys, got)}
    for part in ("frame", "quadrants"):
        for k in keys:
            nan, zero = res[part, True][k], res[part, False][k]
            print(f"{name} K={K} {part} {k}: finite {bool(torch.isfinite(nan).all())}, max |Δ| against the zero-filled run "
                  f"{float((nan - zero).abs().max()):.3e} (rel-L2 {rel_l2(nan.numpy(), zero.numpy()):.3e}), "
                  f"rows with a gradient {int((zero.reshape(zero.shape[0], -1) != 0).any(1).sum())}")
    for part in ("frame", "quadrants"):
        for k in keys:
            nan, zero = res[part, True][k], res[part, False][k]
            assert bool(torch.isfinite(nan).all()) and float(zero.abs().max()) > 0, (part, k)
            assert rel_l2(nan.numpy(), zero.numpy()) <= GRAD_RTOL, (part, k)
    for k in keys:
        assert torch.equal(res["quadrants", True][k], res["quadrants", False][k]), k


# ---- 5. one gradient missing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rest_only", "weight_only"])
def test_a_missing_gradient_equals_explicit_zeros(which, monkeypatch):
    name, K = A, 4
    _P, W, H = hg.REF_CASES[name][:3]
    G, Gr = _g(name, K)
    lib = _lib.load()
    real, seen = lib.ggr_pixel_hits_backward, []

    def spy(st, vw, hp, stream):
        p = hp._obj
        seen.append((bool(p.dL_dweight), bool(p.dL_drest)))
        return real(st, vw, hp, stream)

    monkeypatch.setattr(lib, "ggr_pixel_hits_backward", spy)
    gw, gr = (None, Gr) if which == "rest_only" else (G, None)
    _h, missing = _run(name, K, gw, gr)
    assert seen == [(gw is not None, gr is not None)], "None must travel as NULL"
    _h, zeros = _run(name, K, torch.zeros(K, H, W) if gw is None else gw, torch.zeros(H, W) if gr is None else gr)
    assert seen[-1] == (True, True)
    _close(missing, zeros, GEOM[True], which)


# ---- 6. composition ----------------------------------------------------------------------------------------------------------------
def test_colour_and_hits_in_one_backward_equal_two_backwards():
    name, K = A, 8
    _P, W, H = hg.REF_CASES[name][:3]
    G, Gr = _g(name, K)
    dL = upstream_gradient(W, H, seed=2121).to(DEV)
    col = lambda out: (out[0] * dL).sum()
    _h, both = _run(name, K, G, Gr, more=col)
    _h, g_col = _run(name, K, None, None, more=col)
    _h, g_hit = _run(name, K, G, Gr)
    want = {k: g_col[k] + g_hit[k] for k in both}
    assert all(np.abs(g_col[k]).max() > 0 and np.abs(g_hit[k]).max() > 0 for k in GEOM[True])
    _close(both, want, GEOM[True] + ["shs"], "colour + hits")


def test_features_distortion_and_hits_in_one_backward_equal_three_backwards():
    name, K, KF = Cs, 8, 3
    P, W, H = hg.REF_CASES[name][:3]
    G, Gr = _g(name, K)
    gen = torch.Generator().manual_seed(2131)
    feats = torch.rand(P, KF, generator=gen) * 2.0 - 0.5
    gF, gQ = (torch.randn(KF, H, W, generator=gen) / (H * W)).to(DEV), (torch.randn(H, W, generator=gen) / (H * W)).to(DEV)
    kw = dict(features=feats, return_distortion=True)   # the tuple: colour, radii, depth, features, distortion, hits
    f_loss, d_loss = (lambda out: (out[3] * gF).sum()), (lambda out: (out[4] * gQ).sum())
    _h, all3 = _run(name, K, G, Gr, more=lambda out: f_loss(out) + d_loss(out), **kw)
    parts = [_run(name, K, None, None, more=f_loss, **kw)[1], _run(name, K, None, None, more=d_loss, **kw)[1],
             _run(name, K, G, Gr, **kw)[1]]
    want = {k: parts[0][k] + parts[1][k] + parts[2][k] for k in all3}
    assert all(np.abs(p[k]).max() > 0 for p in parts for k in GEOM[True])
    _close(all3, want, GEOM[True] + ["features"], "features + distortion + hits")
    # … and every pair, in the order the backward chains them
    _h, fh = _run(name, K, G, Gr, more=f_loss, **kw)
    _close(fh, {k: parts[0][k] + parts[2][k] for k in fh}, GEOM[True], "features + hits")
    _h, dh = _run(name, K, G, Gr, more=d_loss, **kw)
    _close(dh, {k: parts[1][k] + parts[2][k] for k in dh}, GEOM[True], "distortion + hits")


# ---- 7. launch sets ----------------------------------------------------------------------------------------------------------------
def test_two_views_of_two_gaussian_sets_equal_per_view_calls():
    from ggrt_official_amd.synthetic import make_scene
    K, P, W, H = 4, 800, 83, 45
    scs = []
    for b in range(2):
        sc = make_scene(P, W, H, sh_degree=1, seed=2141 + b)
        sc.cov3D = sc.cov3D * 0.05
        scs.append(sc.to(DEV))
    gen = torch.Generator().manual_seed(2143)
    G = (torch.randn(4, K, H, W, generator=gen) / (H * W)).to(DEV)
    Gr = (torch.randn(4, H, W, generator=gen) / (H * W)).to(DEV)
    tf = torch.tensor([[scs[0].tanfovx, scs[0].tanfovy]] * 4, dtype=torch.float32, device=DEV)
    rs = scs[0].settings()._replace(sh_max_degree=3, return_hits=K, hits_grad=True)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    cams = [_cams(s, 2) for s in scs]
    view, proj, cam = (torch.cat([c[i] for c in cams]) for i in range(3))
    bg = torch.stack([s.bg for s in scs for _ in range(2)])
    stk = lambda f: leaf(torch.stack([f(s) for s in scs]))
    m, o, c = stk(lambda s: s.means3D), stk(lambda s: s.opacities), stk(lambda s: s.cov3D)
    out = rasterize_views(m, o, view, proj, cam, bg, tf, rs, shs=stk(lambda s: s.shs), cov3D_precomp=c)
    h = out[-1]
    assert h.weight.shape == (4, K, H, W) and h.rest.shape == (4, H, W) and h.weight.requires_grad and h.rest.requires_grad
    assert int(h.count.max()) > K and bool((h.count < K).any())
    ((h.weight * G).sum() + (h.rest * Gr).sum()).backward()
    assert m.grad.shape == (2, P, 3)
    for b, s in enumerate(scs):
        mb, ob, cb = leaf(s.means3D), leaf(s.opacities), leaf(s.cov3D)
        for v in range(2):
            n = 2 * b + v
            r = rs._replace(viewmatrix=view[n], projmatrix=proj[n], campos=cam[n], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            hv = GaussianRasterizer(r)(means3D=mb, means2D=torch.zeros_like(mb), opacities=ob, shs=s.shs, cov3D_precomp=cb)[-1]
            for f in PixelHits._fields:
                assert torch.equal(getattr(hv, f).detach(), getattr(h, f)[n].detach()), (n, f)
            ((hv.weight * G[n]).sum() + (hv.rest * Gr[n]).sum()).backward()
        for a, r_ in zip((m.grad[b], o.grad[b], c.grad[b]), (mb.grad, ob.grad, cb.grad)):
            assert float(r_.abs().max()) > 0 and rel_l2(a.cpu().numpy(), r_.cpu().numpy()) <= GRAD_RTOL


# ---- 8. the scissor ----------------------------------------------------------------------------------------------------------------
def test_scissor_inside_equal_outside_zero():
    name, K = A, 8
    _P, W, H = hg.REF_CASES[name][:3]
    G, Gr = _g(name, K)
    win = (32, 16, 64, 48)   # tile-aligned: tiles x 2..3, y 1..2
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[16:48, 32:64] = True
    h_win, g_win = _run(name, K, G, Gr, scissor=win)
    h_full, g_full = _run(name, K, G * inside, Gr * inside)
    for f in PixelHits._fields:
        a, b = getattr(h_win, f).detach().cpu(), getattr(h_full, f).detach().cpu()
        assert torch.equal(a[..., inside], b[..., inside]), f
        assert bool((a[..., ~inside] == (-1 if f == "index" else 0)).all()), f
    _close(g_win, g_full, GEOM[True], "scissor")
    # a Gaussian that no pixel of the window composited gets nothing
    seen = torch.zeros(hg.REF_CASES[name][0], dtype=torch.bool)
    _out, _l = _forward(name, 32, scissor=win, hits_grad=False)
    if bool((_out[-1].count <= 32).all()):
        seen[_out[-1].index[_out[-1].index >= 0].cpu().long()] = True
        assert not np.any(g_win["opacities"][~seen.numpy()])


# ---- 9. antialiasing ---------------------------------------------------------------------------------------------------------------
def test_antialiasing_matches_the_reference():
    name, K = Cs, 8
    G, Gr = _g(name, K)
    _kw, ref = hg.ref_hits(name, K, antialiasing=True)
    h, grads = _run(name, K, G, Gr, antialiasing=True)
    assert torch.equal(h.index.cpu().to(torch.int64), ref["index"]) and torch.equal(h.count.cpu().to(torch.int64), ref["count"])
    _h, plain = _run(name, K, G, Gr)
    assert rel_l2(grads["opacities"], plain["opacities"]) > 1e-2, "the compensated opacity must matter"
    want = hg.ref_grads(name, K, G, Gr, antialiasing=True)
    for k in GEOM[True]:
        print(f"antialiasing grad {k}: rel-L2 {rel_l2(grads[k], want[k]):.3e}")
    check_grads(grads, want, GEOM[True], tag="hitsgrad:aa")


# ---- 10. modes ---------------------------------------------------------------------------------------------------------------------
def test_a_missed_list_hint_changes_nothing():
    import ggrt_official_amd.rasterizer as R
    name, K = Cs, 8
    P = hg.REF_CASES[name][0]
    G, Gr = _g(name, K)
    R.clear_list_hints()
    h1, g1 = _run(name, K, G, Gr)                          # exact mode (first call of the shape)
    key = next(k for k in R._hints if k[1] == P)
    with R._hint_lock:
        R._hints[key] = [(64, 1)]                           # a guess far too small: the call repairs itself
    before = R.list_hint_stats()["missed"]
    h2, g2 = _run(name, K, G, Gr)
    assert R.list_hint_stats()["missed"] == before + 1
    for f in PixelHits._fields:
        assert torch.equal(getattr(h1, f), getattr(h2, f)), f
    _close(g2, g1, GEOM[True], "missed hint")
    R.clear_list_hints()


def test_sync_free_graph_replay_equals_eager():
    name, K = Cs, 8
    G, Gr = (t.to(DEV) for t in _g(name, K))
    s, kw, leaves = _leaves(name)
    rs = _settings(name, s, leaves, K, hits_grad=True, list_capacity=40_000)
    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)
    rast = GaussianRasterizer(rs)

    def fwd_bwd():
        for t in list(leaves.values()) + [m2d]:
            t.grad = None
        h = rast(means2D=m2d, **kw)[-1]
        ((h.weight * G).sum() + (h.rest * Gr).sum()).backward()
        return h

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_hits = fwd_bwd()
    g_grads = {k: leaves[k].grad for k in GEOM[True]}
    with torch.no_grad():
        leaves["opacities"].mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy().copy() for k, v in g_grads.items()}
    got_w = g_hits.weight.detach().clone()
    # eager, exact mode, on the changed opacities
    e = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    h = GaussianRasterizer(_settings(name, s, e, K, hits_grad=True))(
        means3D=e["means3D"], means2D=torch.zeros_like(e["means3D"]), opacities=e["opacities"], shs=e["shs"],
        cov3D_precomp=e["cov3D_precomp"])[-1]
    ((h.weight * G).sum() + (h.rest * Gr).sum()).backward()
    assert torch.equal(got_w, h.weight.detach())
    _close(got, _np_grads(e), GEOM[True], "graph replay")


def test_a_second_backward_over_one_forward():
    name, K = Cs, 8
    G, Gr = (t.to(DEV) for t in _g(name, K))
    out, leaves = _forward(name, K)
    h = out[-1]
    loss = (h.weight * G).sum() + (h.rest * Gr).sum()
    ins = [leaves[k] for k in GEOM[True]]
    g1 = torch.autograd.grad(loss, ins, retain_graph=True)
    g2 = torch.autograd.grad(loss, ins)
    for a, b in zip(g1, g2):
        assert float(a.abs().max()) > 0 and rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= GRAD_RTOL


def test_gradients_agree_across_the_forms_of_the_depth_sort():
    name, K = A, 8
    G, Gr = _g(name, K)
    h0, base = _run(name, K, G, Gr)
    for sort in ("global", "global_3pass", "per_tile"):
        h, got = _run(name, K, G, Gr, depth_sort=sort)
        for f in PixelHits._fields:
            assert torch.equal(getattr(h, f), getattr(h0, f)), (sort, f)
        _close(got, base, GEOM[True], f"depth_sort={sort}")


# ---- 14. off = the parent ----------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_hit_gradient_call(monkeypatch):
    name, K = Cs, 8
    _P, W, H = hg.REF_CASES[name][:3]
    lib = _lib.load()
    dL = upstream_gradient(W, H, seed=2151).to(DEV)
    col = lambda out: (out[0] * dL).sum()
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_pixel_hits_backward", lambda *a: calls.append("b") or 99)
        h_off, g_off = _run(name, K, None, None, more=col, hits_grad=False)
        assert not h_off.weight.requires_grad and not h_off.rest.requires_grad and h_off.weight.grad_fn is None
        with torch.no_grad():   # on, but no grad mode: as off
            out, _l = _forward(name, K, hits_grad=True)
        assert not out[-1].weight.requires_grad and not out[-1].rest.requires_grad
        for f in PixelHits._fields:
            assert torch.equal(getattr(out[-1], f), getattr(h_off, f)), f
        # on, with a loss that does not touch the hits: no call either
        h_on, g_on = _run(name, K, None, None, more=col, hits_grad=True)
    assert not calls
    assert h_on.weight.requires_grad and h_on.rest.requires_grad
    for f in PixelHits._fields:
        assert torch.equal(getattr(h_on, f).detach(), getattr(h_off, f)), f
    # the colour-only backward is the parent's: same launches with or without the flag (float atomics: within rounding)
    _close(g_on, g_off, GEOM[True] + ["shs"], "off")
    # the detached arrays of an `off` call cannot carry a loss to the geometry
    out, leaves = _forward(name, K, hits_grad=False)
    (composite_hits(leaves["opacities"][:, 0], out[-1]).sum()).backward()
    assert leaves["means3D"].grad is None and leaves["cov3D_precomp"].grad is None
