"""The pick pass on the GPU (`-m gpu`): `return_picks` / ggr_pixel_picks.

Per pixel, over the entries the colour blend composited there: the median-depth Gaussian (the last one in front of which the
transmittance is still > 1/2) and its depth value, the Gaussian of the largest blend weight and that weight, and the number of
entries.  Checked: a closed form, the torch reference on the frozen oracle's lists (tests/picks_reference.py), the contribution
pass and the alpha plane as independent HIP witnesses, the depth value, the invariances, launch sets and the decoder, the
scissor, the sync-free mode under graph capture, "off = as before", and the non-finite contract.

All five planes are order-independent (no sum, no atomic): wherever two HIP runs are compared they are compared with
torch.equal.  The reference scenes are picks_reference.REF_CASES; their seeds were fixed on the CPU (tests/test_picks_reference.py:
the float32 and the float64 reference agree in every pixel), so the caps below are not used up by the reference's own rounding."""
import pytest
import torch

from ggrt_official_amd import (Contributions, GaussianRasterizationSettings, GaussianRasterizer, PixelPicks, _lib, pick_values,
                               rasterize_views)
from ggrt_official_amd.synthetic import make_scene
from tests import picks_reference as pr
from tests.helpers import FLIP_FRACTION, FWD_ATOL, record_metric
from tests.test_gpu_contributions import _hand_camera, _kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANES = PixelPicks._fields


def _run(sc, use_sh=True, use_cov=True, colors=None, train=False, on=True, aux=None, **settings):
    """One GaussianRasterizer call on cuda:0 → the whole returned tuple (picks last when `on`)"""
    s = sc.to(DEV)
    rs = s.settings()._replace(return_picks=on, **settings)
    means = s.means3D.clone().requires_grad_(train)
    extra = {} if aux is None else dict(aux_precomp=aux.to(DEV))
    with torch.enable_grad() if train else torch.no_grad():
        return GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=s.opacities,
                                      **_kw(s, use_sh, use_cov, colors), **extra)


def _same(a, b, tag):
    """two HIP results: every plane bit for bit"""
    for f in PLANES:
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{tag}: {f} differs"


def _scene(seed=991, P=3000, W=96, H=64, D=2):
    return make_scene(P, W, H, sh_degree=D, seed=seed)


def _sparse_scene(seed=992, P=1000):
    """small Gaussians: ≈ 1/6 of the pixels composite nothing and ≈ 1/4 a single entry (measured on the CPU reference)"""
    sc = _scene(seed, P)
    sc.cov3D = sc.cov3D * 0.005
    return sc


# ---- 1. closed form ------------------------------------------------------------------------------------------------------
def test_closed_form_of_four_gaussians_on_the_optical_axis():
    """Four isotropic Gaussians on the optical axis, given out of depth order: z = 4, 2, 5, 3 with opacities 0.3, 0.3, 0.9, 0.3.
    The centre pixel (16, 8) sees α = opacity exactly, so in depth order T_before = 1, 0.7, 0.49, 0.343 and w = 0.3, 0.21,
    0.147, 0.3087: the median is the z = 3 Gaussian (0.7 > 0.5 >= 0.49), the dominant one the z = 5 Gaussian, and neither is
    the first; every decision is >= 2 % from its threshold.  The corners are ≈ 18 px from the axis: nothing reaches them."""
    W, H = 33, 17
    z = torch.tensor([4.0, 2.0, 5.0, 3.0])
    means = torch.stack([torch.zeros(4), torch.zeros(4), z], -1)
    cov6 = torch.tensor([[0.09, 0, 0, 0.09, 0, 0.09]] * 4)
    opac = torch.tensor([[0.3], [0.3], [0.9], [0.3]])
    rs = GaussianRasterizationSettings(**_hand_camera(W, H), return_picks=True)
    with torch.no_grad():
        out = GaussianRasterizer(rs)(means3D=means.to(DEV), means2D=torch.zeros(4, 3, device=DEV), opacities=opac.to(DEV),
                                     colors_precomp=torch.full((4, 3), 0.5, device=DEV), cov3D_precomp=cov6.to(DEV))
    assert len(out) == 4 and isinstance(out[-1], PixelPicks)
    p = out[-1]
    for f in PLANES:
        t = getattr(p, f)
        assert t.shape == (H, W) and t.dtype == (torch.float32 if f in ("median_depth", "max_weight") else torch.int32), f
        assert not t.requires_grad and t.device.type == "cuda"
    assert int(p.median_index[8, 16]) == 3 and float(p.median_depth[8, 16]) == 3.0
    assert int(p.max_index[8, 16]) == 2 and abs(float(p.max_weight[8, 16]) - 0.3087) <= FWD_ATOL
    assert int(p.count[8, 16]) == 4
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert int(p.median_index[y, x]) == -1 and int(p.max_index[y, x]) == -1 and int(p.count[y, x]) == 0
        assert float(p.median_depth[y, x]) == 0.0 and float(p.max_weight[y, x]) == 0.0


# ---- 2. against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.REF_CASES))
def test_against_the_reference_on_the_oracles_lists(name):
    _P, W, H, _D, use_sh, use_cov, aa, _seed = pr.REF_CASES[name]
    sc, colors, ref = pr.ref_case(name, torch.float64)
    out = _run(sc, use_sh, use_cov, colors, antialiasing=aa)
    torch.cuda.synchronize()
    got = {f: getattr(out[-1], f).cpu() for f in PLANES}
    diff = {f: got[f].to(torch.int64) != ref[f] for f in ("median_index", "max_index", "count")}
    any_diff = diff["median_index"] | diff["max_index"] | diff["count"]
    n_diff = {f: int(d.sum()) for f, d in diff.items()}
    agree = ~any_diff
    dw = float((got["max_weight"].double() - ref["max_weight"])[agree].abs().max())
    seen = ref["count"] > 0
    drange = float(ref["median_depth"][seen].max() - ref["median_depth"][seen].min())
    dd = float((got["median_depth"].double() - ref["median_depth"])[agree].abs().max())
    print(f"{name}: pixels differing in median_index {n_diff['median_index']}, max_index {n_diff['max_index']}, count "
          f"{n_diff['count']}, any {int(any_diff.sum())} of {W * H}; max |Δ max_weight| {dw:.3e}; max |Δ median_depth| {dd:.3e} "
          f"over a depth range of {drange:.3f}")
    record_metric(f"picks:ref:{name}", median_index_diff=n_diff["median_index"], max_index_diff=n_diff["max_index"],
                  count_diff=n_diff["count"], any_diff=int(any_diff.sum()), max_weight_abs=dw, median_depth_abs=dd)
    assert int(any_diff.sum()) <= max(FLIP_FRACTION * H * W, 3)
    assert dw <= FWD_ATOL
    assert dd <= FWD_ATOL * drange


# ---- 3. the contribution pass and the alpha plane as witnesses --------------------------------------------------------------
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_two_independent_kernels_agree(which):
    sc = _scene(993) if which == "dense" else _sparse_scene()
    out = _run(sc, return_contributions=True, return_alpha=True)
    assert len(out) == 6 and isinstance(out[4], Contributions) and isinstance(out[5], PixelPicks)
    radii, alpha, con, p = out[1], out[3], out[4], out[5]
    P = radii.shape[0]
    assert int(p.count.sum()) == int(con.pixel_count.sum()) > 10000               # the same integer from two kernels
    assert torch.equal(p.max_weight.max(), con.weight_max.max())                   # bit for bit
    valid = p.max_index >= 0
    per_g = torch.zeros(P, device=DEV).scatter_reduce(0, p.max_index[valid].long(), p.max_weight[valid], "amax")
    assert bool((per_g <= con.weight_max).all())
    none = p.median_index < 0
    assert torch.equal(none, p.count == 0) and torch.equal(none, alpha == 0) and torch.equal(none, p.max_index < 0)
    assert bool((p.max_weight <= alpha + FWD_ATOL).all())
    one = p.count == 1
    assert torch.equal(p.median_index[one], p.max_index[one])
    for idx in (p.median_index, p.max_index):
        assert int(idx.max()) < P and bool((radii[idx[idx >= 0].long()] > 0).all())
    if which == "sparse":
        assert int(none.sum()) > 100 and int(one.sum()) > 100
        assert not p.median_depth[none].any() and not p.max_weight[none].any()
    else:
        assert int(p.count.max()) > 30 and int((p.median_index != p.max_index).sum()) > 100


# ---- 4. the depth value ----------------------------------------------------------------------------------------------------
def test_median_depth_is_the_forwards_depth_value_bit_for_bit():
    from ggrt_official_amd.rasterizer import debug_forward_state
    sc = _sparse_scene()
    s = sc.to(DEV)
    st = debug_forward_state(s.means3D, s.opacities, s.settings(), shs=s.shs, cov3D_precomp=s.cov3D)
    p = _run(sc)[-1]
    assert int((p.median_index >= 0).sum()) > 1000 and int((p.median_index < 0).sum()) > 100
    assert torch.equal(p.median_depth, pick_values(st["depth"], p.median_index))
    aux = torch.rand(s.means3D.shape[0], generator=torch.Generator().manual_seed(994)) * 7 + 0.25
    q = _run(sc, aux=aux)[-1]
    assert torch.equal(q.median_index, p.median_index) and torch.equal(q.max_index, p.max_index)
    assert torch.equal(q.median_depth, pick_values(aux.to(DEV), q.median_index))
    assert not torch.equal(q.median_depth, p.median_depth)


# ---- 5. invariances ------------------------------------------------------------------------------------------------------
def test_invariances():
    import ggrt_official_amd.rasterizer as R
    sc = _scene(995)
    R.clear_list_hints()
    base = _run(sc)                                               # exact mode (first call of the shape)
    assert int(base[-1].count.sum()) > 20000
    _same(_run(sc)[-1], base[-1], "run to run")
    _same(_run(sc, reference_rects=True)[-1], base[-1], "reference rects")
    for form in ("global", "per_tile", "global_3pass"):
        _same(_run(sc, depth_sort=form)[-1], base[-1], f"depth_sort={form}")
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
    scs = [make_scene(P, W, H, sh_degree=2, seed=996 + b).to(DEV) for b in range(2)]
    rs = scs[0].settings()._replace(return_picks=True)

    def per_view(s, view, proj, cam):
        outs = []
        for v in range(view.shape[0]):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            outs.append(GaussianRasterizer(r)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                              shs=s.shs, cov3D_precomp=s.cov3D)[-1])
        return PixelPicks(*(torch.stack([getattr(o, f) for o in outs]) for f in PLANES))

    with torch.no_grad():
        s = scs[0]
        view, proj, cam = _cams(s, 3)
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 3, dtype=torch.float32, device=DEV)
        out = rasterize_views(s.means3D, s.opacities, view, proj, cam, s.bg.reshape(1, 3).expand(3, 3).contiguous(), tf, rs,
                              shs=s.shs, cov3D_precomp=s.cov3D)
        assert len(out) == 4 and all(t.shape == (3, H, W) for t in out[-1])
        assert int(out[-1].count.sum()) > 50000
        _same(out[-1], per_view(s, view, proj, cam), "three views")
        assert not torch.equal(out[-1].median_index[0], out[-1].median_index[2])
        # two Gaussian sets of two views each: the indices are within the view's set
        cams = [_cams(s, 2) for s in scs]
        view, proj, cam = (torch.cat([c[i] for c in cams]) for i in range(3))
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 4, dtype=torch.float32, device=DEV)
        stk = lambda f: torch.stack([f(s) for s in scs])
        out = rasterize_views(stk(lambda s: s.means3D), stk(lambda s: s.opacities), view, proj, cam,
                              torch.stack([scs[v // 2].bg for v in range(4)]), tf, rs._replace(return_contributions=True),
                              shs=stk(lambda s: s.shs), cov3D_precomp=stk(lambda s: s.cov3D))
        assert len(out) == 5 and isinstance(out[3], Contributions) and all(t.shape == (4, H, W) for t in out[-1])
        for idx in (out[-1].median_index, out[-1].max_index):
            assert int(idx.min()) >= -1 and int(idx.max()) < P and int(idx[2:].max()) > P // 2
        assert int(out[-1].count.sum()) == int(out[3].pixel_count.sum())
        for b in range(2):
            _same(PixelPicks(*(t[2 * b:2 * b + 2] for t in out[-1])), per_view(scs[b], *cams[b]), f"set {b}")


def test_decoder_picks_equal_per_view_calls():
    from ggrt_official_amd import splatting as S
    gen = torch.Generator().manual_seed(997)
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
        out = dec(*args, depth_mode="depth", return_picks=True)
        assert plain.picks is None and out.contributions is None and all(t.shape == (b, v, h, w) for t in out.picks)
        assert torch.equal(out.color, plain.color) and torch.equal(out.depth, plain.depth)
        assert int(out.picks.count.sum()) > 20000 and int(out.picks.median_index.max()) < n
        flat = lambda t: t.flatten(0, 1)
        bg = torch.zeros(b * v, 3, device=DEV)
        per_view = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w), bg, gs,
                                        [n_ // v for n_ in range(b * v)], "depth", batched=False, sh_max_degree=3,
                                        return_picks=True)
        assert len(per_view) == 3
        _same(PixelPicks(*(t.reshape(b * v, h, w) for t in out.picks)), per_view[-1], "decoder")
        # with the contributions as well: both, each in its place
        both = dec(*args, depth_mode="depth", return_picks=True, return_contributions=True, return_alpha=True)
        _same(both.picks, out.picks, "decoder, with contributions")
        assert int(both.picks.count.sum()) == int(both.contributions.pixel_count.sum()) and both.alpha is not None
        # the reference-shaped call site takes the keyword too, with and without a depth pass
        slow = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=False).to(DEV)
        o2 = slow(*args, depth_mode="depth", return_picks=True)
        o3 = slow(*args, return_picks=True, return_contributions=True, return_alpha=True)
        assert all(t.shape == (b, v, h, w) for t in o2.picks) and o3.alpha is not None and o2.contributions is None
        for f in ("median_index", "max_index", "max_weight", "count"):   # (the depth VALUE differs: o2's pass blends the depth feature)
            assert torch.equal(getattr(o3.picks, f), getattr(o2.picks, f)), f
        assert int(o3.picks.count.sum()) == int(o3.contributions.pixel_count.sum())


# ---- 7. scissor ----------------------------------------------------------------------------------------------------------
def test_scissor_inside_equal_outside_none():
    sc = _scene(998)
    x0, y0, x1, y1 = 16, 16, 64, 48                    # tile-aligned: the window's tiles are exactly its pixels
    full, win = _run(sc)[-1], _run(sc, scissor=(x0, y0, x1, y1))[-1]
    inside = torch.zeros(64, 96, dtype=torch.bool, device=DEV)
    inside[y0:y1, x0:x1] = True
    assert int(full.count[~inside].sum()) > 10000 and int(full.count[inside].sum()) > 10000
    for f in PLANES:
        a, b = getattr(win, f), getattr(full, f)
        assert torch.equal(a[inside], b[inside]), f
        none = -1 if f.endswith("index") else 0
        assert bool((a[~inside] == none).all()), f


# ---- 8. sync-free mode under graph capture ---------------------------------------------------------------------------------
def test_sync_free_graph_replay_equals_eager():
    sc = _scene(999)
    s = sc.to(DEV)
    rs = s.settings()._replace(list_capacity=400_000, return_picks=True)
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
    before = g_out[-1].median_index.clone()
    op.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = GaussianRasterizer(s.settings()._replace(return_picks=True))
    with torch.no_grad():
        e_out = eager(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=op, shs=s.shs, cov3D_precomp=s.cov3D)
    assert torch.equal(g_out[0], e_out[0]) and int(e_out[-1].count.sum()) > 20000
    _same(g_out[-1], e_out[-1], "graph replay")
    assert not torch.equal(before, g_out[-1].median_index)      # (the replay did see the new opacities)


# ---- 9. off is off -----------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_pick_call(monkeypatch):
    lib = _lib.load()
    sc = _scene(1000)
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_pixel_picks", lambda *a: calls.append("p") or 99)
        off = _run(sc, on=False)
        off_train = _run(sc, on=False, train=True)
        off_contrib = _run(sc, on=False, return_contributions=True)
        with pytest.raises(RuntimeError, match="ggr_pixel_picks"):
            _run(sc)                                      # (the patch is in the path of an "on" call)
    assert len(off) == 3 and len(off_train) == 3 and len(off_contrib) == 4 and calls == ["p"]
    on = _run(sc)
    assert len(on) == 4 and isinstance(on[-1], PixelPicks)
    for a, b in zip(off, on[:3]):
        assert torch.equal(a, b)
    on_all = _run(sc, return_alpha=True, return_contributions=True)
    assert len(on_all) == 6 and isinstance(on_all[-2], Contributions) and isinstance(on_all[-1], PixelPicks)
    assert on_all[3].shape == (64, 96) and torch.equal(on_all[-2].pixel_count, off_contrib[-1].pixel_count)


# ---- 10. the non-finite contract ---------------------------------------------------------------------------------------------
def test_a_nan_mean_is_in_no_index_plane_and_changes_nothing_else():
    sc = _scene(1001)
    full = _run(sc)[-1]
    ids, n = torch.unique(full.median_index[full.median_index >= 0], return_counts=True)
    g = int(ids[n.argmax()])                    # the Gaussian that is the median of the most pixels
    bad = sc.to("cpu")
    bad.means3D = bad.means3D.clone()
    bad.means3D[g, 1] = float("nan")
    got = _run(bad)
    assert int(got[1][g]) == 0
    got = got[-1]
    assert not bool((got.median_index == g).any()) and not bool((got.max_index == g).any())
    keep = torch.arange(3000) != g
    rest = sc.to("cpu")
    for f in ("means3D", "cov3D", "scales", "rotations", "opacities", "shs"):
        setattr(rest, f, getattr(rest, f)[keep])
    want = _run(rest)[-1]
    reindex = lambda idx: idx - (idx > g).to(idx.dtype)       # (−1 stays −1)
    assert torch.equal(reindex(got.median_index), want.median_index) and torch.equal(reindex(got.max_index), want.max_index)
    for f in ("median_depth", "max_weight", "count"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert not torch.equal(got.median_index, full.median_index)   # (the removed Gaussian was picked somewhere)
