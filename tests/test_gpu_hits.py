"""The hit pass on the GPU (`-m gpu`): `return_hits` / ggr_pixel_hits.

Per pixel, the first K list entries the colour blend composited there, in list order, with their blend weights, the sum of the
weights behind the K-th, and the number of all of them.  Checked: a closed form, the torch reference on the frozen oracle's lists
(tests/hits_reference.py), the pick pass, the contribution pass, the alpha plane and the feature pass as independent HIP
witnesses, truncation, the invariances, launch sets and the decoder, the scissor, the sync-free mode under graph capture,
"off = as before", the non-finite contract, and the C host's slots-only form of the call on long lists.

No array comes from an atomic or a cross-lane sum (`rest` is a per-pixel sum in list order): wherever two HIP runs are compared
they are compared with torch.equal.  The reference scenes are hits_reference.REF_CASES; their seeds were fixed on the CPU
(tests/test_hits_reference.py: the float32 and the float64 reference agree in every pixel), so the cap below is not used up by the
reference's own rounding."""
import ctypes as C

import pytest
import torch

from ggrt_official_amd import (Contributions, GaussianRasterizationSettings, GaussianRasterizer, PixelHits, PixelPicks, _lib,
                               composite_hits, rasterize_views)
from ggrt_official_amd.synthetic import make_scene
from tests import hits_reference as hr
from tests.helpers import FLIP_FRACTION, FWD_ATOL, record_metric
from tests.test_gpu_contributions import _hand_camera, _kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARRAYS = PixelHits._fields


def _run(sc, K=8, use_sh=True, use_cov=True, colors=None, train=False, features=None, **settings):
    """One GaussianRasterizer call on cuda:0 → the whole returned tuple (hits last when K > 0)"""
    s = sc.to(DEV)
    rs = s.settings()._replace(return_hits=K, **settings)
    means = s.means3D.clone().requires_grad_(train)
    extra = {} if features is None else dict(features_precomp=features.to(DEV))
    with torch.enable_grad() if train else torch.no_grad():
        return GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=s.opacities,
                                      **_kw(s, use_sh, use_cov, colors), **extra)


def _same(a, b, tag):
    """two HIP results: every array bit for bit"""
    for f in ARRAYS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{tag}: {f} differs"


def _scene(seed=1991, P=3000, W=96, H=64, D=2):
    return make_scene(P, W, H, sh_degree=D, seed=seed)


def _sparse_scene():
    """hits_reference's third scene — small Gaussians: on the CPU reference no pixel composites more than 9 entries, 1801 at
    least 3 and 967 none"""
    return hr.ref_case("C_small_gaussians_unfilled_slots", torch.float32)[0]


def _well_formed(h, K, P):
    """what holds for every PixelHits: the slots are filled from the front, exactly min(count, K) of them, padding is −1 / 0"""
    valid = h.index >= 0
    assert int(h.index.min()) >= -1 and int(h.index.max()) < P
    assert torch.equal(valid.sum(-3).to(torch.int32), h.count.clamp(max=K))
    assert bool((valid[..., 1:, :, :] <= valid[..., :-1, :, :]).all())
    assert bool((h.weight[~valid] == 0).all()) and bool((h.index[~valid] == -1).all()) and bool((h.weight[valid] > 0).all())
    assert bool((h.rest[h.count <= K] == 0).all()) and bool((h.rest >= 0).all())


# ---- 1. closed form ------------------------------------------------------------------------------------------------------
def test_closed_form_of_four_gaussians_on_the_optical_axis():
    """Four isotropic Gaussians on the optical axis, given out of depth order: z = 4, 2, 5, 3 with opacities 0.3, 0.3, 0.9, 0.3.
    The centre pixel (16, 8) sees α = opacity exactly, so in depth order — ids 1, 3, 0, 2 — T_before = 1, 0.7, 0.49, 0.343 and
    w = 0.3, 0.21, 0.147, 0.3087.  The corners are ≈ 18 px from the axis: nothing reaches them."""
    W, H = 33, 17
    z = torch.tensor([4.0, 2.0, 5.0, 3.0])
    means = torch.stack([torch.zeros(4), torch.zeros(4), z], -1)
    cov6 = torch.tensor([[0.09, 0, 0, 0.09, 0, 0.09]] * 4)
    opac = torch.tensor([[0.3], [0.3], [0.9], [0.3]])
    corners = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))

    def call(K):
        rs = GaussianRasterizationSettings(**_hand_camera(W, H), return_hits=K)
        with torch.no_grad():
            out = GaussianRasterizer(rs)(means3D=means.to(DEV), means2D=torch.zeros(4, 3, device=DEV), opacities=opac.to(DEV),
                                         colors_precomp=torch.full((4, 3), 0.5, device=DEV), cov3D_precomp=cov6.to(DEV))
        assert len(out) == 4 and isinstance(out[-1], PixelHits)
        h = out[-1]
        assert h.index.shape == h.weight.shape == (K, H, W) and h.rest.shape == h.count.shape == (H, W)
        assert h.index.dtype == h.count.dtype == torch.int32 and h.weight.dtype == h.rest.dtype == torch.float32
        assert all(t.device.type == "cuda" and not t.requires_grad for t in h)
        for y, x in corners:
            assert bool((h.index[:, y, x] == -1).all()) and bool((h.weight[:, y, x] == 0).all())
            assert float(h.rest[y, x]) == 0.0 and int(h.count[y, x]) == 0
        _well_formed(h, K, 4)
        return h

    w_all = [0.3, 0.21, 0.147, 0.3087]
    h = call(2)
    assert h.index[:, 8, 16].tolist() == [1, 3]
    assert all(abs(float(h.weight[k, 8, 16]) - w_all[k]) <= FWD_ATOL for k in range(2))
    assert abs(float(h.rest[8, 16]) - (0.147 + 0.3087)) <= FWD_ATOL and int(h.count[8, 16]) == 4
    h = call(4)
    assert h.index[:, 8, 16].tolist() == [1, 3, 0, 2] and float(h.rest[8, 16]) == 0.0 and int(h.count[8, 16]) == 4
    assert all(abs(float(h.weight[k, 8, 16]) - w_all[k]) <= FWD_ATOL for k in range(4))
    h = call(6)
    assert h.index[:, 8, 16].tolist() == [1, 3, 0, 2, -1, -1] and h.weight[4:, 8, 16].tolist() == [0.0, 0.0]
    assert float(h.rest[8, 16]) == 0.0 and int(h.count[8, 16]) == 4


# ---- 2. against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hr.REF_CASES))
def test_against_the_reference_on_the_oracles_lists(name):
    _P, W, H, _D, use_sh, use_cov, aa, _seed = hr.REF_CASES[name]
    K = hr.REF_K
    sc, colors, ref, _picks = hr.ref_case(name, torch.float64)
    out = _run(sc, K, use_sh, use_cov, colors, antialiasing=aa)
    torch.cuda.synchronize()
    got = {f: getattr(out[-1], f).cpu() for f in ARRAYS}
    slot_diff = (got["index"].to(torch.int64) != ref["index"]).any(0)
    count_diff = got["count"].to(torch.int64) != ref["count"]
    any_diff = slot_diff | count_diff
    agree = ~any_diff
    dw = float((got["weight"].double() - ref["weight"])[:, agree].abs().max())
    dr = float((got["rest"].double() - ref["rest"])[agree].abs().max())
    print(f"{name}: pixels differing in a slot index {int(slot_diff.sum())}, in count {int(count_diff.sum())}, any "
          f"{int(any_diff.sum())} of {W * H}; max |Δ weight| {dw:.3e}; max |Δ rest| {dr:.3e}")
    record_metric(f"hits:ref:{name}", slot_diff=int(slot_diff.sum()), count_diff=int(count_diff.sum()),
                  any_diff=int(any_diff.sum()), weight_abs=dw, rest_abs=dr)
    assert int(any_diff.sum()) <= max(FLIP_FRACTION * H * W, 3)
    assert dw <= FWD_ATOL
    assert dr <= FWD_ATOL


# ---- 3. independent HIP witnesses ------------------------------------------------------------------------------------------
def test_pick_contribution_alpha_and_feature_passes_agree():
    K, C_ = 16, 5
    sc = _sparse_scene()
    P = sc.means3D.shape[0]
    feat = torch.rand(P, C_, generator=torch.Generator().manual_seed(1992))
    out = _run(sc, K, features=feat, return_picks=True, return_contributions=True, return_alpha=True)
    assert len(out) == 8 and isinstance(out[5], Contributions) and isinstance(out[6], PixelPicks) and isinstance(out[7], PixelHits)
    alpha, planes, con, p, h = out[3], out[4], out[5], out[6], out[7]
    # not vacuous: every pixel's whole list is in its slots, and many pixels have several entries
    assert int(h.count.max()) <= K
    assert int((h.count >= 3).sum()) >= 1000
    _well_formed(h, K, P)
    assert not h.rest.any()                                                         # == 0 exactly
    assert torch.equal(h.count, p.count)
    wmax, first = h.weight.max(0)
    assert torch.equal(wmax, p.max_weight)                                          # the blend's own bits, from two kernels
    first = (h.weight == wmax[None]).to(torch.int32).argmax(0)                      # the earliest slot that holds the maximum
    assert torch.equal(h.index.gather(0, first[None].long())[0], p.max_index)
    assert float((h.weight.sum(0) - alpha).abs().max()) <= FWD_ATOL
    valid = h.index >= 0
    assert torch.equal(torch.bincount(h.index[valid].long(), minlength=P).to(torch.int32), con.pixel_count)
    wsum = torch.zeros(P, device=DEV).index_add_(0, h.index[valid].long(), h.weight[valid])
    assert float((wsum - con.weight_sum).abs().max()) <= FWD_ATOL * float(con.weight_sum.max())
    wtop = torch.zeros(P, device=DEV).scatter_reduce(0, h.index[valid].long(), h.weight[valid], "amax")
    assert torch.equal(wtop, con.weight_max)
    comp = composite_hits(feat.to(DEV), h)
    assert comp.shape == (sc.height, sc.width, C_)
    assert float((comp.permute(2, 0, 1) - planes).abs().max()) <= FWD_ATOL


# ---- 4. truncation -----------------------------------------------------------------------------------------------------
def test_truncation_on_the_dense_scene():
    sc = _scene(1993)
    P = sc.means3D.shape[0]
    h16, h3 = _run(sc, 16)[-1], _run(sc, 3)[-1]
    assert int((h16.count > 16).sum()) > 1000                                       # (dense: the slots are filled, a rest is left)
    _well_formed(h16, 16, P)
    _well_formed(h3, 3, P)
    assert torch.equal(h3.index, h16.index[:3]) and torch.equal(h3.weight, h16.weight[:3])
    assert torch.equal(h3.count, h16.count)
    assert float((h3.rest - (h16.weight[3:].sum(0) + h16.rest)).abs().max()) <= FWD_ATOL
    h1, h32 = _run(sc, 1)[-1], _run(sc, _lib.MAX_HITS)[-1]
    assert h1.index.shape == (1, 64, 96) and h32.index.shape == (32, 64, 96)
    _well_formed(h1, 1, P)
    _well_formed(h32, 32, P)
    assert torch.equal(h1.index, h16.index[:1]) and torch.equal(h1.weight, h16.weight[:1]) and torch.equal(h1.count, h16.count)
    assert torch.equal(h32.index[:16], h16.index) and torch.equal(h32.weight[:16], h16.weight) and torch.equal(h32.count, h16.count)


# ---- 5. invariances ------------------------------------------------------------------------------------------------------
def test_invariances():
    import ggrt_official_amd.rasterizer as R
    sc = _scene(1995)
    R.clear_list_hints()
    base = _run(sc)                                               # exact mode (first call of the shape)
    assert int(base[-1].count.sum()) > 20000 and float(base[-1].rest.max()) > 0.1
    _same(_run(sc)[-1], base[-1], "run to run")
    _same(_run(sc, reference_rects=True)[-1], base[-1], "reference rects")
    for form in ("global", "per_tile", "global_3pass"):
        _same(_run(sc, depth_sort=form)[-1], base[-1], f"depth_sort={form}")
    train = _run(sc, train=True)
    assert train[0].requires_grad and not any(x.requires_grad for x in train[-1])
    _same(train[-1], base[-1], "training forward")
    train[0].sum().backward()                                      # the backward over the same buffers still runs
    R.clear_list_hints()


# ---- 6. launch sets and the decoder --------------------------------------------------------------------------------------
def test_launch_set_and_gaussian_sets_equal_per_view_calls():
    from tests.test_gpu_alpha import _cams
    P, W, H, K = 2500, 96, 64, 4
    scs = [make_scene(P, W, H, sh_degree=2, seed=1996 + b).to(DEV) for b in range(2)]
    rs = scs[0].settings()._replace(return_hits=K)

    def per_view(s, view, proj, cam):
        outs = []
        for v in range(view.shape[0]):
            r = rs._replace(viewmatrix=view[v], projmatrix=proj[v], campos=cam[v], bg=s.bg, tanfovx=s.tanfovx, tanfovy=s.tanfovy)
            outs.append(GaussianRasterizer(r)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                              shs=s.shs, cov3D_precomp=s.cov3D)[-1])
        return PixelHits(*(torch.stack([getattr(o, f) for o in outs]) for f in ARRAYS))

    with torch.no_grad():
        s = scs[0]
        view, proj, cam = _cams(s, 3)
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 3, dtype=torch.float32, device=DEV)
        out = rasterize_views(s.means3D, s.opacities, view, proj, cam, s.bg.reshape(1, 3).expand(3, 3).contiguous(), tf, rs,
                              shs=s.shs, cov3D_precomp=s.cov3D)
        assert len(out) == 4 and isinstance(out[-1], PixelHits)
        assert out[-1].index.shape == out[-1].weight.shape == (3, K, H, W) and out[-1].rest.shape == out[-1].count.shape == (3, H, W)
        assert int(out[-1].count.sum()) > 50000
        _same(out[-1], per_view(s, view, proj, cam), "three views")
        assert not torch.equal(out[-1].index[0], out[-1].index[2])
        # two Gaussian sets of two views each: the indices are within the view's set
        cams = [_cams(s, 2) for s in scs]
        view, proj, cam = (torch.cat([c[i] for c in cams]) for i in range(3))
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * 4, dtype=torch.float32, device=DEV)
        stk = lambda f: torch.stack([f(s) for s in scs])
        out = rasterize_views(stk(lambda s: s.means3D), stk(lambda s: s.opacities), view, proj, cam,
                              torch.stack([scs[v // 2].bg for v in range(4)]), tf, rs._replace(return_picks=True),
                              shs=stk(lambda s: s.shs), cov3D_precomp=stk(lambda s: s.cov3D))
        assert len(out) == 5 and isinstance(out[3], PixelPicks) and out[-1].index.shape == (4, K, H, W)
        assert int(out[-1].index.min()) >= -1 and int(out[-1].index.max()) < P and int(out[-1].index[2:].max()) > P // 2
        assert torch.equal(out[-1].count, out[3].count)
        for b in range(2):
            _same(PixelHits(*(t[2 * b:2 * b + 2] for t in out[-1])), per_view(scs[b], *cams[b]), f"set {b}")


def test_decoder_hits_equal_per_view_calls():
    from ggrt_official_amd import splatting as S
    gen = torch.Generator().manual_seed(1997)
    b, v, n, d_sh, h, w, K = 2, 2, 2000, 9, 64, 96, 4
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
        out = dec(*args, depth_mode="depth", return_hits=K)
        assert plain.hits is None and out.picks is None and out.contributions is None
        assert out.hits.index.shape == out.hits.weight.shape == (b, v, K, h, w)
        assert out.hits.rest.shape == out.hits.count.shape == (b, v, h, w)
        assert torch.equal(out.color, plain.color) and torch.equal(out.depth, plain.depth)
        assert int(out.hits.count.sum()) > 20000 and int(out.hits.index.max()) < n
        flat = lambda t: t.flatten(0, 1)
        bg = torch.zeros(b * v, 3, device=DEV)
        per_view = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w), bg, gs,
                                        [n_ // v for n_ in range(b * v)], "depth", batched=False, sh_max_degree=3,
                                        return_hits=K)
        assert len(per_view) == 3
        _same(PixelHits(*(flat(t) for t in out.hits)), per_view[-1], "decoder")
        # with the picks and the contributions as well: all three, each in its place
        every = dec(*args, depth_mode="depth", return_hits=K, return_picks=True, return_contributions=True, return_alpha=True)
        _same(every.hits, out.hits, "decoder, with picks and contributions")
        assert torch.equal(every.hits.count, every.picks.count) and every.alpha is not None
        assert int(every.hits.count.sum()) == int(every.contributions.pixel_count.sum())
        # the reference-shaped call site takes the keyword too, with and without a depth pass
        slow = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=False).to(DEV)
        o2 = slow(*args, depth_mode="depth", return_hits=K)
        o3 = slow(*args, return_hits=K, return_picks=True, return_alpha=True)
        assert o2.hits.index.shape == (b, v, K, h, w) and o3.alpha is not None and o2.picks is None
        _same(o3.hits, o2.hits, "reference-shaped call site")
        assert torch.equal(o3.hits.count, o3.picks.count)


# ---- 7. scissor ----------------------------------------------------------------------------------------------------------
def test_scissor_inside_equal_outside_padding():
    sc = _scene(1998)
    x0, y0, x1, y1 = 16, 16, 64, 48                    # tile-aligned: the window's tiles are exactly its pixels
    full, win = _run(sc)[-1], _run(sc, scissor=(x0, y0, x1, y1))[-1]
    inside = torch.zeros(64, 96, dtype=torch.bool, device=DEV)
    inside[y0:y1, x0:x1] = True
    assert int(full.count[~inside].sum()) > 10000 and int(full.count[inside].sum()) > 10000
    for f in ARRAYS:
        a, b = getattr(win, f), getattr(full, f)
        assert torch.equal(a[..., inside], b[..., inside]), f
        assert bool((a[..., ~inside] == (-1 if f == "index" else 0)).all()), f


# ---- 8. sync-free mode under graph capture ---------------------------------------------------------------------------------
def test_sync_free_graph_replay_equals_eager():
    sc = _scene(1999)
    s = sc.to(DEV)
    rs = s.settings()._replace(list_capacity=400_000, return_hits=8)
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
    graph.replay()
    torch.cuda.synchronize()
    before = g_out[-1].weight.clone()
    op.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = GaussianRasterizer(s.settings()._replace(return_hits=8))
    with torch.no_grad():
        e_out = eager(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=op, shs=s.shs, cov3D_precomp=s.cov3D)
    assert torch.equal(g_out[0], e_out[0]) and int(e_out[-1].count.sum()) > 20000
    _same(g_out[-1], e_out[-1], "graph replay")
    assert not torch.equal(before, g_out[-1].weight)      # (the second replay did see the new opacities)


# ---- 9. off is off -----------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical_and_makes_no_hit_call(monkeypatch):
    lib = _lib.load()
    sc = _scene(2000)
    s = sc.to(DEV)

    class Unaware(tuple):
        """a settings object that never heard of `return_hits`: the tuple's fields as attributes, nothing else"""
        def __getattr__(self, name):
            fields = GaussianRasterizationSettings._fields
            if name in fields:
                return self[fields.index(name)]
            raise AttributeError(name)

    def call(rs, train=False):
        means = s.means3D.clone().requires_grad_(train)
        with torch.enable_grad() if train else torch.no_grad():
            return GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=s.opacities, shs=s.shs,
                                          cov3D_precomp=s.cov3D)

    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(lib, "ggr_pixel_hits", lambda *a: calls.append("h") or 99)
        old = call(Unaware(s.settings()))
        off = call(s.settings()._replace(return_hits=0))
        off_train = call(s.settings(), train=True)
        off_picks = call(s.settings()._replace(return_picks=True, return_contributions=True, return_alpha=True))
        with pytest.raises(RuntimeError, match="ggr_pixel_hits"):
            _run(sc)                                      # (the patch is in the path of an "on" call)
    assert len(old) == len(off) == len(off_train) == 3 and len(off_picks) == 6 and calls == ["h"]
    for a, b, c in zip(old, off, off_train):
        assert torch.equal(a, b) and torch.equal(a, c.detach())
    on = _run(sc)
    assert len(on) == 4 and isinstance(on[-1], PixelHits)
    for a, b in zip(off, on[:3]):
        assert torch.equal(a, b)
    on_all = _run(sc, return_alpha=True, return_contributions=True, return_picks=True)
    assert len(on_all) == 7 and isinstance(on_all[-3], Contributions) and isinstance(on_all[-2], PixelPicks)
    assert isinstance(on_all[-1], PixelHits)
    for a, b in zip(off_picks[:4], on_all[:4]):
        assert torch.equal(a, b)
    for a, b in zip(off_picks[5], on_all[5]):
        assert torch.equal(a, b)
    assert torch.equal(on_all[4].pixel_count, off_picks[4].pixel_count) and torch.equal(on_all[4].weight_max, off_picks[4].weight_max)


# ---- 10. the non-finite contract ---------------------------------------------------------------------------------------------
def test_a_nan_mean_is_in_no_slot_and_changes_nothing_else():
    sc = _scene(2001)
    P = sc.means3D.shape[0]
    full = _run(sc)[-1]
    ids, n = torch.unique(full.index[full.index >= 0], return_counts=True)
    g = int(ids[n.argmax()])                    # the Gaussian that sits in the most slots
    for what in (float("nan"), float("inf")):
        bad = sc.to("cpu")
        bad.means3D = bad.means3D.clone()
        bad.means3D[g, 1] = what
        got = _run(bad)
        assert int(got[1][g]) == 0
        got = got[-1]
        assert not bool((got.index == g).any())
        assert int(got.index.min()) >= -1 and int(got.index.max()) < P
        keep = torch.arange(P) != g
        rest = sc.to("cpu")
        for f in ("means3D", "cov3D", "scales", "rotations", "opacities", "shs"):
            setattr(rest, f, getattr(rest, f)[keep])
        want = _run(rest)[-1]
        reindex = lambda idx: idx - (idx > g).to(idx.dtype)       # (−1 stays −1)
        assert torch.equal(reindex(got.index), want.index)
        for f in ("weight", "rest", "count"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f
        assert not torch.equal(got.index, full.index)   # (the removed Gaussian was in some slot)
        _well_formed(got, 8, P)


# ---- 11. the slots-only form of the C call on long lists -----------------------------------------------------------------------
def test_slots_only_call_equals_the_full_call_on_multi_batch_lists():
    """A C host may pass out_rest = out_count = NULL; a pixel is then finished once it holds K entries and the walk ends early.
    On the reference scene with lists of more than two staging batches that must not change a byte of index / weight."""
    import ggrt_official_amd.rasterizer as R
    lib = _lib.load()
    sc, _colors, _ref, _picks = hr.ref_case("A_sh_cov", torch.float64)
    s = sc.to(DEV)
    P, H, W, K = s.means3D.shape[0], sc.height, sc.width, 5

    class _Ctx:  # minimal stand-in for the autograd ctx: keeps the forward's buffers
        def set_materialize_grads(self, v): pass
        def save_for_backward(self, *t): self.saved = t
        def mark_non_differentiable(self, *t): pass

    ctx = _Ctx()
    rs = s.settings()._replace(return_hits=K)
    with torch.no_grad():
        out = R._RasterizeGaussians.forward(ctx, s.means3D, torch.zeros_like(s.means3D), s.shs, None, s.opacities, None, None,
                                            s.cov3D, rs.viewmatrix, rs.projmatrix, rs.campos, None, rs)
    full = PixelHits(*out[-4:])
    geom, img, binb = ctx.saved[12], ctx.saved[13], ctx.saved[14]
    st = R._settings_struct(rs, P, ctx.dims[1], ctx.saved[7], ctx.saved[8], ctx.saved[9], ctx.saved[10])
    idx = torch.full((K, H, W), 77, dtype=torch.int32, device=DEV)
    wgt = torch.full((K, H, W), 77.0, dtype=torch.float32, device=DEV)
    hp = _lib.hit_pass(num_hits=K, geom_buffer=geom.data_ptr(), image_buffer=img.data_ptr(), binning_buffer=binb.data_ptr(),
                       num_rendered=ctx.num_rendered, out_index=idx.data_ptr(), out_weight=wgt.data_ptr(), out_rest=None,
                       out_count=None)
    rc = lib.ggr_pixel_hits(C.byref(st), None, C.byref(hp), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert int((full.count > K).sum()) > H * W // 2
    assert torch.equal(idx, full.index) and torch.equal(wgt, full.weight)
