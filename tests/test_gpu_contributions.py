"""The contribution pass on the GPU (`-m gpu`): `return_contributions` / ggr_contributions.

Per Gaussian, over the pixels where the colour blend composited it: Σ w, max w (w = α·T) and the number of those pixels.
Checked: a closed form, occlusion (what `radii` cannot tell), the torch reference on the frozen oracle's lists
(tests/contributions_reference.py), the feature pass and the alpha plane as independent HIP witnesses, the invariances, launch
sets and the decoder, the scissor, the sync-free mode under graph capture, "off = as before", and the non-finite contract.

weight_max and pixel_count are compared bit for bit wherever two HIP runs are compared (integer atomics of order-independent
values); weight_sum is a float sum added atomically in varying order and goes through helpers.check_grads, like a gradient row.

The reference scenes (REF_CASES) were chosen on the CPU: for each of them the reference computed in float32 and in float64
gives the SAME pixel_count in every row and weight_max within helpers.FWD_ATOL (measured: 0 of 215-364 k live pairs differ,
max |Δ weight_max| <= 1.9e-6), so the caps of the comparison are not used up by the reference's own rounding.  Seeds 931-936
were tried per configuration; the first that passed this check was taken: A 931, B 931, C 931."""
import numpy as np
import pytest
import torch

from ggrt_official_amd import Contributions, GaussianRasterizer, _lib, rasterize_views
from ggrt_official_amd.synthetic import make_scene
from tests import contributions_reference as cr
from tests.helpers import FLIP_FRACTION, FWD_ATOL, check_grads, record_metric

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(c):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy() for t in c)


def _kw(s, use_sh, use_cov, colors):
    kw = dict(shs=s.shs) if use_sh else dict(colors_precomp=colors.to(DEV))
    kw.update(dict(cov3D_precomp=s.cov3D) if use_cov else dict(scales=s.scales, rotations=s.rotations))
    return kw


def _run(sc, use_sh=True, use_cov=True, colors=None, train=False, on=True, **settings):
    """One GaussianRasterizer call on cuda:0 → the whole returned tuple (contributions last when `on`)"""
    s = sc.to(DEV)
    rs = s.settings()._replace(return_contributions=on, **settings)
    means = s.means3D.clone().requires_grad_(train)
    with torch.enable_grad() if train else torch.no_grad():
        return GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=s.opacities,
                                      **_kw(s, use_sh, use_cov, colors))


def _same(a, b, tag):
    """two HIP results: max and count bit for bit, the sum like a gradient row"""
    a, b = _np(a), _np(b)
    assert np.array_equal(a[1], b[1]), f"{tag}: weight_max differs"
    assert np.array_equal(a[2], b[2]), f"{tag}: pixel_count differs"
    check_grads(dict(weight_sum=a[0]), dict(weight_sum=b[0]), ["weight_sum"], tag=f"contrib:{tag}")


def _scene(seed=941, P=3000, W=96, H=64, D=2):
    return make_scene(P, W, H, sh_degree=D, seed=seed)


# ---- 1. closed form ------------------------------------------------------------------------------------------------------
def _hand_camera(W, H):
    tanx, tany = 1.0, H / W
    zn, zf = 1.0, 100.0
    proj = torch.tensor([[2 * zn * 0.5 / tanx, 0, 0, 0], [0, 2 * zn * 0.5 / tany, 0, 0], [0, 0, zf / (zf - zn), 1],
                         [0, 0, -(zf * zn) / (zf - zn), 0]], dtype=torch.float32)
    return dict(image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4), projmatrix=proj, sh_degree=0, campos=torch.zeros(3), prefiltered=False)


def _hand_call(W, H, means, cov6, opac, **settings):
    from ggrt_official_amd import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(**_hand_camera(W, H), return_contributions=True, **settings)
    P = means.shape[0]
    with torch.no_grad():
        return GaussianRasterizer(rs)(means3D=means.to(DEV), means2D=torch.zeros(P, 3, device=DEV), opacities=opac.to(DEV),
                                      colors_precomp=torch.full((P, 3), 0.5, device=DEV), cov3D_precomp=cov6.to(DEV))


def test_closed_form_of_one_centred_gaussian():
    """One isotropic Gaussian of opacity 0.8 on the optical axis over nothing: T = 1 everywhere, α(d) = 0.8·exp(−d²/(2σ²)) with
    σ² = (focal/z)²·0.09 + 0.3 = 1.8314 px²; d² is an integer and the threshold d² = 2σ²·ln(0.8·255) = 19.48 lies between 18
    and 20 — no pixel centre within 2 % of it.  The other Gaussians stand behind the camera."""
    W, H, P, g = 33, 17, 5, 2
    means = torch.tensor([[0.1 * i, 0.0, -3.0] for i in range(P)])
    means[g] = torch.tensor([0.0, 0.0, 4.0])
    cov6 = torch.tensor([[0.09, 0, 0, 0.09, 0, 0.09]] * P)
    out = _hand_call(W, H, means, cov6, torch.full((P, 1), 0.8))
    assert len(out) == 4 and isinstance(out[-1], Contributions)
    wsum, wmax, count = _np(out[-1])
    assert wsum.dtype == np.float32 and wmax.dtype == np.float32 and count.dtype == np.int32 and count.shape == (P,)
    var2d = (0.5 * W / 4.0) ** 2 * 0.09 + 0.3
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    d2 = (xs - 16) ** 2 + (ys - 8) ** 2
    alpha = np.minimum(0.99, 0.8 * np.exp(-0.5 * d2 / var2d))
    live = alpha >= 1.0 / 255.0
    assert np.abs(alpha[~live] * 255 - 1).min() > 1e-4 and np.abs(alpha[live] * 255 - 1).min() > 1e-4
    assert abs(wmax[g] - min(0.99, 0.8 * np.exp(-0.5 * d2.min() / var2d))) <= FWD_ATOL
    assert count[g] == int(live.sum()) == 61
    assert abs(wsum[g] - alpha[live].sum()) <= 1e-4 * alpha[live].sum()
    others = np.arange(P) != g
    assert not wsum[others].any() and not wmax[others].any() and not count[others].any()
    assert not _np((out[1],))[0][others].any()


# ---- 2. occlusion: what radii cannot tell ------------------------------------------------------------------------------
def test_gaussians_behind_an_opaque_surface_have_radii_but_no_contribution():
    """Three dense layers of opacity-0.99 Gaussians (σ ≈ 3 px on a 4-px grid reaching 40 px beyond the frame: every pixel has a
    centre within 2.9 px in each layer, α >= 0.62 from that one alone, several more above 0.3 — T falls below 1e-4 inside the
    second layer) stand in front of 400 Gaussians spread over the frame."""
    W, H = 64, 48
    focal = 0.5 * W   # tanfovx = 1
    front = []
    for layer in range(3):
        z = 3.0 + 0.01 * layer
        px, py = torch.meshgrid(torch.arange(-40.0, W + 41, 4), torch.arange(-40.0, H + 41, 4), indexing="xy")
        x = (px.reshape(-1) - (W - 1) / 2) / focal * z
        y = (py.reshape(-1) - (H - 1) / 2) / focal * z
        front.append(torch.stack([x, y, torch.full_like(x, z)], -1))
    front = torch.cat(front)
    gen = torch.Generator().manual_seed(951)
    nb, zb = 400, 6.0
    bx = (torch.rand(nb, generator=gen) * (W - 1) - (W - 1) / 2) / focal * zb
    by = (torch.rand(nb, generator=gen) * (H - 1) - (H - 1) / 2) / focal * zb
    back = torch.stack([bx, by, torch.full((nb,), zb)], -1)
    means = torch.cat([front, back])
    nf = front.shape[0]
    var_f, var_b = (3.0 / focal * 3.0) ** 2, (2.0 / focal * zb) ** 2
    cov6 = torch.zeros(nf + nb, 6)
    cov6[:nf, 0] = cov6[:nf, 3] = cov6[:nf, 5] = var_f
    cov6[nf:, 0] = cov6[nf:, 3] = cov6[nf:, 5] = var_b
    out = _hand_call(W, H, means, cov6, torch.full((nf + nb, 1), 0.99))
    radii = out[1].cpu().numpy()
    wsum, wmax, count = _np(out[-1])
    assert (radii[nf:] > 0).all()
    assert not count[nf:].any() and not wmax[nf:].any() and not wsum[nf:].any()
    assert (count[:nf] > 0).sum() > 500 and wmax[:nf].max() > 0.3   # (the in-frame part of the front layer; equal depths blend in index order)
    assert int(count.sum()) >= W * H        # every pixel composited something


# ---- 3. against the reference ------------------------------------------------------------------------------------------
REF_CASES = {   # P, W, H, D, use_sh, use_cov, antialiasing, seed
    "A_sh_cov": (3000, 96, 64, 3, True, True, False, 931),
    "B_colours_scale_rot_aa_odd_frame": (3000, 83, 45, 1, False, False, True, 931),
    "C_sh_scale_rot": (2500, 96, 64, 2, True, False, False, 931),
}


@pytest.mark.parametrize("name", list(REF_CASES))
def test_against_the_reference_on_the_oracles_lists(name):
    P, W, H, D, use_sh, use_cov, aa, seed = REF_CASES[name]
    sc = make_scene(P, W, H, sh_degree=D, seed=seed)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    ref = [t.numpy() for t in cr.scene_contributions(sc, use_sh, use_cov, colors, aa, torch.float64)]
    out = _run(sc, use_sh, use_cov, colors, antialiasing=aa)
    wsum, wmax, count = _np(out[-1])
    dmax = float(np.abs(wmax - ref[1]).max())
    dcount = int(np.abs(count.astype(np.int64) - ref[2]).sum())
    print(f"{name}: max |Δ weight_max| {dmax:.3e}, Σ|Δ pixel_count| {dcount} of {int(ref[2].sum())}")
    record_metric(f"contrib:ref:{name}", max_abs=dmax, count_diff=dcount, pairs=int(ref[2].sum()))
    assert int(ref[2].sum()) > 20000 and int((ref[2] > 0).sum()) > P // 10
    check_grads(dict(weight_sum=wsum), dict(weight_sum=ref[0]), ["weight_sum"], tag=f"contrib:ref:{name}")
    assert dmax <= FWD_ATOL
    assert dcount <= FLIP_FRACTION * int(ref[2].sum())
    seen, radii = ref[2] > 0, out[1].cpu().numpy()
    assert (radii[seen] > 0).all() and not count[radii == 0].any()


# ---- 4. the feature pass and the alpha plane as witnesses ----------------------------------------------------------------
def test_weight_sum_equals_the_feature_gradient_and_adds_up_to_alpha():
    sc = _scene(942)
    s = sc.to(DEV)
    ones = torch.ones(3000, 1, device=DEV, requires_grad=True)
    rs = s.settings()._replace(return_contributions=True, return_alpha=True)
    means = s.means3D.clone().requires_grad_(True)
    out = GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=s.opacities, shs=s.shs,
                                 cov3D_precomp=s.cov3D, features_precomp=ones)
    assert len(out) == 6 and out[4].shape == (1, 64, 96) and isinstance(out[5], Contributions)
    assert not any(t.requires_grad for t in out[5])
    out[4].sum().backward()
    wsum = _np(out[5])[0]
    check_grads(dict(weight_sum=wsum), dict(weight_sum=ones.grad[:, 0].cpu().numpy()), ["weight_sum"], tag="contrib:features")
    a, b = float(wsum.astype(np.float64).sum()), float(out[3].detach().double().sum())
    record_metric("contrib:alpha", rel=abs(a - b) / b)
    print(f"Σ weight_sum {a:.6f}, Σ alpha {b:.6f}, rel {abs(a - b) / b:.3e}")
    assert b > 1000 and abs(a - b) <= 1e-4 * b


# ---- 5. invariances ------------------------------------------------------------------------------------------------------
def test_invariances():
    import ggrt_official_amd.rasterizer as R
    sc = _scene(943)
    R.clear_list_hints()
    base = _run(sc)                                               # exact mode (first call of the shape)
    assert int(_np(base[-1])[2].sum()) > 20000
    _same(_run(sc)[-1], base[-1], "run to run")
    _same(_run(sc, reference_rects=True)[-1], base[-1], "reference rects")
    g, t = _run(sc, depth_sort="global"), _run(sc, depth_sort="per_tile")
    _same(g[-1], t[-1], "global against per-tile sort")
    _same(g[-1], base[-1], "explicit sort")
    train = _run(sc, train=True)
    assert train[0].requires_grad and not any(x.requires_grad for x in train[-1])
    _same(train[-1], base[-1], "training forward")
    train[0].sum().backward()                                      # the backward over the same buffers still runs
    # a deliberately missed list hint: the call repairs itself and the pass runs on the lists it finally returned
    R.clear_list_hints()
    first = _run(sc)
    key = next(k for k in R._hints if k[1] == 3000)
    with R._hint_lock:
        R._hints[key] = [(64, 1)]
    before = R.list_hint_stats()["missed"]
    again = _run(sc)
    assert R.list_hint_stats()["missed"] == before + 1
    _same(again[-1], first[-1], "missed list hint")
    assert torch.equal(again[0], first[0])
    R.clear_list_hints()


# ---- 6. launch sets and the decoder --------------------------------------------------------------------------------------
def test_launch_set_and_gaussian_sets_equal_per_view_calls():
    from tests.test_gpu_alpha import _cams
    P, W, H = 2500, 96, 64
    scs = [make_scene(P, W, H, sh_degree=2, seed=961 + b).to(DEV) for b in range(2)]
    rs = scs[0].settings()._replace(return_contributions=True)

    def per_view(s, view, proj, cam):
        outs = []
        for v in range(view.shape[0]):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            outs.append(GaussianRasterizer(r)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                              shs=s.shs, cov3D_precomp=s.cov3D)[-1])
        return Contributions(*(torch.stack([getattr(o, f) for o in outs]) for f in Contributions._fields))

    with torch.no_grad():
        s = scs[0]
        view, proj, cam = _cams(s, 3)
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 3, dtype=torch.float32, device=DEV)
        out = rasterize_views(s.means3D, s.opacities, view, proj, cam, s.bg.reshape(1, 3).expand(3, 3).contiguous(), tf, rs,
                              shs=s.shs, cov3D_precomp=s.cov3D)
        assert len(out) == 4 and all(t.shape == (3, P) for t in out[-1])
        assert int(out[-1].pixel_count.sum()) > 50000
        _same(out[-1], per_view(s, view, proj, cam), "three views")
        # two Gaussian sets of two views each
        cams = [_cams(s, 2) for s in scs]
        view, proj, cam = (torch.cat([c[i] for c in cams]) for i in range(3))
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 4, dtype=torch.float32, device=DEV)
        stk = lambda f: torch.stack([f(s) for s in scs])
        out = rasterize_views(stk(lambda s: s.means3D), stk(lambda s: s.opacities), view, proj, cam,
                              torch.stack([scs[v // 2].bg for v in range(4)]), tf, rs, shs=stk(lambda s: s.shs),
                              cov3D_precomp=stk(lambda s: s.cov3D))
        assert all(t.shape == (4, P) for t in out[-1])
        for b in range(2):
            _same(Contributions(*(t[2 * b:2 * b + 2] for t in out[-1])), per_view(scs[b], *cams[b]), f"set {b}")


def test_decoder_contributions_equal_per_view_calls():
    from ggrt_official_amd import splatting as S
    gen = torch.Generator().manual_seed(971)
    b, v, n, d_sh, h, w = 2, 2, 2000, 9, 64, 96
    ext = torch.eye(4).repeat(b, v, 1, 1)
    ext[..., 0, 3] = torch.linspace(-0.2, 0.2, v)
    Kmat = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    means = torch.randn(b, n, 3, generator=gen) * torch.tensor([0.6, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(b, n, 3, 3, generator=gen) * 0.05
    cov = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3)
    harm = torch.randn(b, n, 3, d_sh, generator=gen) * 0.3
    opac = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    to = lambda t: t.to(DEV)
    gs = S.Gaussians(to(means), to(cov), to(harm), to(opac))
    args = (gs, to(ext), to(Kmat), to(near), to(far), (h, w))
    dec = S.DecoderSplattingCUDA(sh_max_degree=3).to(DEV)
    with torch.no_grad():
        plain = dec(*args, depth_mode="depth")
        out = dec(*args, depth_mode="depth", return_contributions=True)
        assert plain.contributions is None and all(t.shape == (b, v, n) for t in out.contributions)
        assert torch.equal(out.color, plain.color) and torch.equal(out.depth, plain.depth)
        assert int(out.contributions.pixel_count.sum()) > 20000
        flat = lambda t: t.flatten(0, 1)
        bg = torch.zeros(b * v, 3, device=DEV)
        per_view = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w), bg, gs,
                                        [n_ // v for n_ in range(b * v)], "depth", batched=False, sh_max_degree=3,
                                        return_contributions=True)
        assert len(per_view) == 3
        _same(Contributions(*(t.reshape(b * v, n) for t in out.contributions)), per_view[-1], "decoder")
        # the reference-shaped call site takes the keyword too, with and without a depth pass
        slow = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=False).to(DEV)
        o2 = slow(*args, depth_mode="depth", return_contributions=True)
        o3 = slow(*args, return_contributions=True, return_alpha=True)
        assert all(t.shape == (b, v, n) for t in o2.contributions) and o3.alpha is not None
        _same(o3.contributions, o2.contributions, "reference-shaped call site")
        keep = S.contribution_keep_mask(out.contributions)
        assert keep.shape == (b, n) and torch.equal(keep, out.contributions.pixel_count.amax(1) > 0)


# ---- 7. scissor ----------------------------------------------------------------------------------------------------------
def test_scissor_outside_zero_inside_equal():
    from ggrt_official_amd.rasterizer import debug_forward_state
    sc = _scene(944)
    s = sc.to(DEV)
    st = debug_forward_state(s.means3D, s.opacities, s.settings(), shs=s.shs, cov3D_precomp=s.cov3D)
    xy, r = st["xy"].cpu().numpy(), st["radii"].cpu().numpy().astype(np.float64)
    x0, y0, x1, y1 = 16, 16, 64, 48                    # tile-aligned: the window's tiles are exactly its pixels
    full = _np(_run(sc)[-1])
    win = _np(_run(sc, scissor=(x0, y0, x1, y1))[-1])
    lo_x, hi_x, lo_y, hi_y = xy[:, 0] - r - 1, xy[:, 0] + r + 1, xy[:, 1] - r - 1, xy[:, 1] + r + 1
    vis = r > 0
    inside = vis & (lo_x >= x0) & (hi_x <= x1 - 1) & (lo_y >= y0) & (hi_y <= y1 - 1)
    outside = vis & ((hi_x < x0) | (lo_x > x1 - 1) | (hi_y < y0) | (lo_y > y1 - 1))
    assert (full[2][inside] > 0).sum() > 20 and (full[2][outside] > 0).sum() > 50
    for k in range(3):
        assert not win[k][outside].any()
    assert np.array_equal(win[1][inside], full[1][inside]) and np.array_equal(win[2][inside], full[2][inside])
    check_grads(dict(weight_sum=win[0][inside]), dict(weight_sum=full[0][inside]), ["weight_sum"], tag="contrib:scissor")
    assert (win[2] <= full[2]).all() and (win[1] <= full[1]).all()


# ---- 8. sync-free mode under graph capture ---------------------------------------------------------------------------------
def test_sync_free_graph_replay_equals_eager():
    sc = _scene(945)
    s = sc.to(DEV)
    rs = s.settings()._replace(list_capacity=400_000, return_contributions=True)
    op = s.opacities.clone()
    rast = GaussianRasterizer(rs)

    def fwd():
        with torch.no_grad():
            return rast(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=op, shs=s.shs, cov3D_precomp=s.cov3D)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = fwd()
    op.mul_(0.8)
    graph.replay()
    torch.cuda.synchronize()
    eager = GaussianRasterizer(s.settings()._replace(return_contributions=True))
    with torch.no_grad():
        e_out = eager(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=op, shs=s.shs, cov3D_precomp=s.cov3D)
    assert torch.equal(g_out[0], e_out[0]) and int(e_out[-1].pixel_count.sum()) > 20000
    _same(g_out[-1], e_out[-1], "graph replay")


# ---- 9. off is off -----------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_contribution_call(monkeypatch):
    lib = _lib.load()
    sc = _scene(946)
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_contributions", lambda *a: calls.append("c") or 99)
        off = _run(sc, on=False)
        off_train = _run(sc, on=False, train=True)
        with pytest.raises(RuntimeError, match="ggr_contributions"):
            _run(sc)                                      # (the patch is in the path of an "on" call)
    assert len(off) == 3 and len(off_train) == 3 and calls == ["c"]
    on = _run(sc)
    assert len(on) == 4
    for a, b in zip(off, on[:3]):
        assert torch.equal(a, b)
    on_alpha = _run(sc, return_alpha=True)
    assert len(on_alpha) == 5 and isinstance(on_alpha[-1], Contributions) and on_alpha[3].shape == (64, 96)


# ---- 10. the non-finite contract ---------------------------------------------------------------------------------------------
def test_a_nan_mean_has_zeros_and_changes_no_other_row():
    sc = _scene(947)
    full = _np(_run(sc)[-1])
    g = int(np.argmax(full[2]))                 # the most visible Gaussian
    bad = sc.to("cpu")
    bad.means3D = bad.means3D.clone()
    bad.means3D[g, 1] = float("nan")
    got = _run(bad)
    assert int(got[1][g]) == 0
    got = _np(got[-1])
    assert got[0][g] == 0 and got[1][g] == 0 and got[2][g] == 0
    keep = torch.arange(3000) != g
    rest = sc.to("cpu")
    for f in ("means3D", "cov3D", "scales", "rotations", "opacities", "shs"):
        setattr(rest, f, getattr(rest, f)[keep])
    want = _np(_run(rest)[-1])
    k = keep.numpy()
    assert np.array_equal(got[1][k], want[1]) and np.array_equal(got[2][k], want[2])
    assert not np.array_equal(want[1], full[1][k])          # (the removed Gaussian did stand in front of others: their T rose)
    check_grads(dict(weight_sum=got[0][k]), dict(weight_sum=want[0]), ["weight_sum"], tag="contrib:nonfinite")
