"""`return_hits`, `PixelHits` and `composite_hits` — the call surface, no GPU."""
import copy
import inspect
import pickle

import pytest
import torch

import ggrt_official_amd as g
from ggrt_official_amd import _lib
from ggrt_official_amd import splatting as S
from tests.test_picks_settings import _kw


def test_return_hits_rides_beside_the_settings_tuple():
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "return_hits" not in S0._fields
    off, on = S0(**_kw()), S0(**_kw(), return_hits=4)
    assert off.return_hits == 0 and on.return_hits == 4 and type(on.return_hits) is int
    assert on.return_picks is False and on.return_contributions is False
    assert len(on) == len(off) == len(S0._fields) and tuple(on)[:4] == tuple(off)[:4]
    assert tuple.__eq__(on._replace(bg=None, viewmatrix=None, projmatrix=None, campos=None),
                        off._replace(bg=None, viewmatrix=None, projmatrix=None, campos=None))      # equality: the tuple's
    assert on._replace(sh_max_degree=4).return_hits == 4 and on._replace(sh_max_degree=4).sh_max_degree == 4
    assert off._replace(return_hits=7).return_hits == 7 and off.return_hits == 0
    both = on._replace(return_picks=True)
    assert both.return_hits == 4 and both.return_picks is True and both._replace(return_hits=0).return_picks is True
    assert both._replace(return_hits=0).return_hits == 0
    assert on._asdict()["return_hits"] == 4 and off._asdict()["return_hits"] == 0
    assert list(on._asdict())[:len(S0._fields)] == list(S0._fields)
    assert "return_hits=4" in repr(on) and "return_hits=0" in repr(off)
    assert repr(on).endswith("return_contributions=False, return_picks=False)")
    # positional construction is what it was: the tuple's fields, then return_contributions, then return_picks — no slot for K
    assert S0(*off).return_hits == 0 and S0(*off, True, True).return_hits == 0
    with pytest.raises(TypeError):
        S0(*off, False, False, 4)
    assert S0(*off, return_hits=2).return_hits == 2
    assert S0._make(list(on)).return_hits == 0
    assert copy.copy(on).return_hits == 4 and pickle.loads(pickle.dumps(on)).return_hits == 4


@pytest.mark.parametrize("bad", [-1, _lib.MAX_HITS + 1, 1.5, True, "4", None])
def test_a_value_outside_the_range_raises(bad):
    S0 = g.GaussianRasterizationSettings
    with pytest.raises(ValueError, match="return_hits"):
        S0(**_kw(), return_hits=bad)
    with pytest.raises(ValueError, match="return_hits"):
        S0(**_kw())._replace(return_hits=bad)


def test_the_limits_are_accepted():
    S0 = g.GaussianRasterizationSettings
    assert _lib.MAX_HITS == 32
    assert S0(**_kw(), return_hits=1).return_hits == 1 and S0(**_kw(), return_hits=_lib.MAX_HITS).return_hits == 32


def test_exports_and_call_site_keywords():
    assert g.PixelHits._fields == ("index", "weight", "rest", "count")
    assert "PixelHits" in g.__all__ and "composite_hits" in g.__all__ and S.PixelHits is g.PixelHits
    for fn in (S.render_cuda, S.render_color_and_depth, S.render_views_fused, S.DecoderSplattingCUDA.forward, S.boundary_arguments):
        p = inspect.signature(fn).parameters
        assert "return_hits" in p and p["return_hits"].default == 0 and p["return_hits"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        names = list(p)                                     # (keyword-only, in front of the two keyword-only flags: no
        assert names[-3:] == ["return_hits", "return_picks", "return_contributions"]   # positional parameter has moved)
        n_pos = sum(q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for q in p.values())
        with pytest.raises(TypeError):
            fn(*([None] * n_pos), 4)
    c, d = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert S.DecoderOutput(c, d).hits is None and S.DecoderOutput(c, d, d, c, None, None).hits is None
    assert S._fused_result(c, d, None, False, None, None, "p", "h") == (c, d, "p", "h")
    assert S._fused_result(c, d, None, False, c, "x", None, "h") == (c, d, c, "x", "h")
    assert S._tail_index(True, True, True) == (-4, -3) and S._tail_index(True, True) == (-3, -2) and S._pick_index(4) == -2


def test_the_public_tuple_ends_with_the_hits():
    from ggrt_official_amd.rasterizer import _with_contributions
    raw = tuple(range(3 + 3 + 5 + 4))
    out = _with_contributions(raw, True, True, True)
    assert len(out) == 6 and isinstance(out[3], g.Contributions) and isinstance(out[4], g.PixelPicks) and isinstance(out[5], g.PixelHits)
    assert tuple(out[3]) == (3, 4, 5) and tuple(out[4]) == (6, 7, 8, 9, 10) and tuple(out[5]) == (11, 12, 13, 14)
    out = _with_contributions(tuple(range(7)), False, False, True)
    assert out[:3] == (0, 1, 2) and tuple(out[3]) == (3, 4, 5, 6)
    assert _with_contributions(tuple(range(8)), False, True) == (0, 1, 2, g.PixelPicks(3, 4, 5, 6, 7))     # (as it was)


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
        if rs.return_hits:
            K = rs.return_hits
            out += (g.PixelHits(torch.full((K, H, W), 13, dtype=torch.int32), torch.full((K, H, W), 14.0), torch.full((H, W), 15.0),
                                torch.full((H, W), 16, dtype=torch.int32)),)
        return out


@pytest.mark.parametrize("fused_inputs", [True, False])
@pytest.mark.parametrize("depth_mode", [None, "depth"])
@pytest.mark.parametrize("alpha,feat,contrib,picks", [(False, False, False, False), (True, True, True, True), (False, True, False, True),
                                                      (True, False, True, False)])
def test_call_site_layer_hands_every_element_to_its_place(monkeypatch, fused_inputs, depth_mode, alpha, feat, contrib, picks):
    """The decoder's three paths (per-view fused call, colour + depth in one pass, the reference-shaped colour pass) with a stub
    in the rasterizer's place: whatever else is on, `.hits` gets the hits and every other field what it got before."""
    monkeypatch.setattr(S, "GaussianRasterizer", _StubRasterizer)
    b, v, n, h, w, K = 2, 2, 7, 4, 6, 3
    ext = torch.eye(4).repeat(b, v, 1, 1)
    Kmat = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    gs = S.Gaussians(torch.randn(b, n, 3) + torch.tensor([0.0, 0.0, 4.0]), torch.eye(3).repeat(b, n, 1, 1) * 0.01,
                     torch.zeros(b, n, 3, 9), torch.full((b, n), 0.5))
    dec = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=fused_inputs)
    kw = dict(depth_mode=depth_mode, return_alpha=alpha, gaussian_features=torch.zeros(b, n, 5) if feat else None,
              return_picks=picks, return_contributions=contrib)
    out = dec(gs, ext, Kmat, near, far, (h, w), return_hits=K, **kw)
    assert out.color.shape == (b, v, 3, h, w) and bool((out.color == 1).all())
    assert (out.alpha is not None) == alpha and (not alpha or (out.alpha.shape == (b, v, h, w) and bool((out.alpha == 3).all())))
    assert (out.features is not None) == feat and (not feat or (out.features.shape == (b, v, 5, h, w) and bool((out.features == 4).all())))
    assert (out.contributions is not None) == contrib and (out.picks is not None) == picks
    if contrib:
        assert [float(t.flatten()[0]) for t in out.contributions] == [5.0, 6.0, 7.0] and out.contributions.weight_sum.shape == (b, v, n)
    if picks:
        assert isinstance(out.picks, g.PixelPicks) and all(t.shape == (b, v, h, w) for t in out.picks)
        assert [float(t.flatten()[0]) for t in out.picks] == [8.0, 9.0, 10.0, 11.0, 12.0]
    assert isinstance(out.hits, g.PixelHits)
    assert out.hits.index.shape == out.hits.weight.shape == (b, v, K, h, w) and out.hits.rest.shape == out.hits.count.shape == (b, v, h, w)
    assert [float(t.flatten()[0]) for t in out.hits] == [13.0, 14.0, 15.0, 16.0]
    off = dec(gs, ext, Kmat, near, far, (h, w), **kw)
    assert off.hits is None and (off.picks is not None) == picks and (off.contributions is not None) == contrib
    assert (off.features is not None) == feat
