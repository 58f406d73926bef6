"""`return_picks`, `PixelPicks` and `pick_values` — the call surface, no GPU."""
import copy
import inspect
import pickle

import pytest
import torch

import ggrt_official_amd as g
from ggrt_official_amd import splatting as S


def _kw():
    e = torch.eye(4)
    return dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=e,
                projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False)


def test_return_picks_rides_beside_the_settings_tuple():
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "return_picks" not in S0._fields
    off, on = S0(**_kw()), S0(**_kw(), return_picks=True)
    assert off.return_picks is False and on.return_picks is True and on.return_contributions is False
    assert len(on) == len(off) == len(S0._fields) and tuple(on)[:4] == tuple(off)[:4]
    assert on._replace(sh_max_degree=4).return_picks is True and on._replace(sh_max_degree=4).sh_max_degree == 4
    assert off._replace(return_picks=True).return_picks is True and off.return_picks is False
    both = on._replace(return_contributions=True)
    assert both.return_picks is True and both.return_contributions is True
    assert both._replace(return_picks=False).return_contributions is True and both._replace(return_picks=False).return_picks is False
    assert on._asdict()["return_picks"] is True and off._asdict()["return_picks"] is False
    assert list(on._asdict())[:len(S0._fields)] == list(S0._fields)
    assert repr(on).endswith("return_contributions=False, return_picks=True)") and "return_picks=False" in repr(off)
    # positional construction: the tuple's fields as always, then return_contributions, then return_picks
    assert S0(*off).return_picks is False and S0(*off, True).return_picks is False
    assert S0(*off, False, True).return_picks is True and S0(*off, False, True).return_contributions is False
    assert S0._make(list(on)).return_picks is False
    assert copy.copy(on).return_picks is True and pickle.loads(pickle.dumps(on)).return_picks is True


def test_exports_and_call_site_keywords():
    import diff_gaussian_rasterization as dgr
    assert g.PixelPicks._fields == ("median_depth", "median_index", "max_weight", "max_index", "count")
    assert dgr.PixelPicks is g.PixelPicks and dgr.pick_values is g.pick_values and S.PixelPicks is g.PixelPicks
    assert dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**_kw(), return_picks=True))._settings_for_call().return_picks is True
    for fn in (S.render_cuda, S.render_color_and_depth, S.render_views_fused, S.DecoderSplattingCUDA.forward):
        p = inspect.signature(fn).parameters
        assert "return_picks" in p and p["return_picks"].default is False, fn
        # both trailing flags are keyword-only: return_picks stands where return_contributions' positional slot was, and a
        # positional value there must fail loudly instead of switching the wrong pass on
        assert p["return_picks"].kind is inspect.Parameter.KEYWORD_ONLY and p["return_contributions"].kind is inspect.Parameter.KEYWORD_ONLY
        n_pos = sum(q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for q in p.values())
        with pytest.raises(TypeError):
            fn(*([None] * n_pos), True)
    c, d = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert S.DecoderOutput(c, d).picks is None and S.DecoderOutput(c, d, d, c, None).picks is None
    assert S._fused_result(c, d, None, False, None, None, "p") == (c, d, "p")
    assert S._fused_result(c, d, None, False, c, "x", "p") == (c, d, c, "x", "p")


def test_pick_values_fills_and_routes_the_gradient_to_the_picked_rows():
    index = torch.tensor([[2, -1, 4], [4, 0, -1]], dtype=torch.int32)
    v = torch.arange(6, dtype=torch.float32).mul(1.5).requires_grad_(True)
    out = g.pick_values(v, index, fill=-3.0)
    assert out.shape == (2, 3) and out.dtype == torch.float32
    assert torch.equal(out.detach(), torch.tensor([[3.0, -3.0, 6.0], [6.0, 0.0, -3.0]]))
    (out * torch.tensor([[1.0, 10.0, 100.0], [1000.0, 2.0, 20.0]])).sum().backward()
    assert torch.equal(v.grad, torch.tensor([2.0, 0.0, 1.0, 0.0, 1100.0, 0.0]))      # exactly the picked rows; −1 gives nothing
    m = torch.arange(12, dtype=torch.float64).reshape(6, 2).requires_grad_(True)
    out = g.pick_values(m, index)
    assert out.shape == (2, 3, 2) and out.dtype == torch.float64
    assert torch.equal(out[0, 0].detach(), m[2].detach()) and torch.equal(out[0, 1].detach(), torch.zeros(2, dtype=torch.float64))
    out.sum().backward()
    assert torch.equal(m.grad, torch.tensor([[1.0, 1], [0, 0], [1, 1], [0, 0], [2, 2], [0, 0]], dtype=torch.float64))
    assert torch.equal(g.pick_values(v.detach(), torch.full((3,), -1)), torch.zeros(3))
    with pytest.raises(ValueError):
        g.pick_values(torch.zeros(2, 2, 2), index)


class _StubRasterizer:
    """Stands in for GaussianRasterizer on the CPU: returns the tuple the settings ask for, every element tagged by its place"""

    def __init__(self, settings):
        self.rs = settings

    def __call__(self, means3D, means2D, opacities, features_precomp=None, **kw):
        rs, P = self.rs, means3D.shape[0]
        H, W = rs.image_height, rs.image_width
        out = (torch.full((3, H, W), 1.0), torch.ones(P, dtype=torch.int32), torch.full((H, W), 2.0))
        if rs.return_alpha:
            out += (torch.full((H, W), 3.0),)
        if features_precomp is not None:
            out += (torch.full((features_precomp.shape[1], H, W), 4.0),)
        if rs.return_contributions:
            out += (g.Contributions(torch.full((P,), 5.0), torch.full((P,), 6.0), torch.full((P,), 7, dtype=torch.int32)),)
        if rs.return_picks:
            out += (g.PixelPicks(torch.full((H, W), 8.0), torch.full((H, W), 9, dtype=torch.int32), torch.full((H, W), 10.0),
                                 torch.full((H, W), 11, dtype=torch.int32), torch.full((H, W), 12, dtype=torch.int32)),)
        return out


@pytest.mark.parametrize("fused_inputs", [True, False])
@pytest.mark.parametrize("depth_mode", [None, "depth"])
@pytest.mark.parametrize("alpha,feat,contrib", [(False, False, False), (True, True, True), (False, True, False), (True, False, True)])
def test_call_site_layer_hands_every_element_to_its_place(monkeypatch, fused_inputs, depth_mode, alpha, feat, contrib):
    """The decoder's three paths (per-view fused call, colour + depth in one pass, the reference-shaped colour pass) with a stub
    in the rasterizer's place: whatever else is on, `.picks` gets the picks and every other field what it got before."""
    monkeypatch.setattr(S, "GaussianRasterizer", _StubRasterizer)
    b, v, n, h, w = 2, 2, 7, 4, 6
    ext = torch.eye(4).repeat(b, v, 1, 1)
    Kmat = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    gs = S.Gaussians(torch.randn(b, n, 3) + torch.tensor([0.0, 0.0, 4.0]), torch.eye(3).repeat(b, n, 1, 1) * 0.01,
                     torch.zeros(b, n, 3, 9), torch.full((b, n), 0.5))
    dec = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=fused_inputs)
    out = dec(gs, ext, Kmat, near, far, (h, w), depth_mode=depth_mode, return_alpha=alpha,
              gaussian_features=torch.zeros(b, n, 5) if feat else None, return_picks=True, return_contributions=contrib)
    assert out.color.shape == (b, v, 3, h, w) and bool((out.color == 1).all())
    assert (out.alpha is not None) == alpha and (not alpha or (out.alpha.shape == (b, v, h, w) and bool((out.alpha == 3).all())))
    assert (out.features is not None) == feat and (not feat or (out.features.shape == (b, v, 5, h, w) and bool((out.features == 4).all())))
    assert (out.contributions is not None) == contrib
    if contrib:
        assert [float(t.flatten()[0]) for t in out.contributions] == [5.0, 6.0, 7.0] and out.contributions.weight_sum.shape == (b, v, n)
    assert isinstance(out.picks, g.PixelPicks) and all(t.shape == (b, v, h, w) for t in out.picks)
    assert [float(t.flatten()[0]) for t in out.picks] == [8.0, 9.0, 10.0, 11.0, 12.0]
    off = dec(gs, ext, Kmat, near, far, (h, w), depth_mode=depth_mode, return_alpha=alpha,
              gaussian_features=torch.zeros(b, n, 5) if feat else None, return_contributions=contrib)
    assert off.picks is None and (off.contributions is not None) == contrib and (off.features is not None) == feat
