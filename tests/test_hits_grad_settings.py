"""`hits_grad` — the call surface, no GPU."""
import copy
import inspect
import pickle

import pytest
import torch

import ggrt_official_amd as g
from ggrt_official_amd import splatting as S


def _kw():
    z = torch.zeros(3)
    return dict(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=z, scale_modifier=1.0, viewmatrix=torch.eye(4),
                projmatrix=torch.eye(4), sh_degree=0, campos=z, prefiltered=False)


def test_hits_grad_rides_beside_the_settings_tuple():
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "hits_grad" not in S0._fields
    kw = _kw()   # (the same tensor objects in both: the tuples compare by identity)
    off, on = S0(**kw, return_hits=4), S0(**kw, return_hits=4, hits_grad=True)
    assert off.hits_grad is False and on.hits_grad is True and S0(**_kw()).hits_grad is False
    assert len(on) == len(off) == len(S0._fields) and tuple(on) == tuple(off) and on == off   # (not an item of the tuple)
    assert on._replace(sh_max_degree=4).hits_grad is True and on._replace(sh_max_degree=4).return_hits == 4
    assert off._replace(hits_grad=True).hits_grad is True and off.hits_grad is False
    assert on._replace(hits_grad=False).hits_grad is False and on._replace(hits_grad=False).return_hits == 4
    assert on._replace(return_hits=7).hits_grad is True and on._replace(return_hits=7).return_hits == 7
    assert S0(**_kw())._replace(return_hits=2, hits_grad=True).hits_grad is True
    assert on._replace(return_hits=0, hits_grad=False).return_hits == 0
    assert on._asdict()["hits_grad"] is True and off._asdict()["hits_grad"] is False
    assert set(on._asdict()) - set(S0._fields) >= {"hits_grad", "return_hits", "absgrad"}
    assert "hits_grad=True" in repr(on) and "hits_grad=False" in repr(off)
    assert S0(*off).hits_grad is False and S0(*off, True, True).hits_grad is False            # positional construction as it was
    assert S0(*off, return_hits=2, hits_grad=True).hits_grad is True
    assert S0._make(list(on)).hits_grad is False
    assert copy.copy(on).hits_grad is True and pickle.loads(pickle.dumps(on)).hits_grad is True
    both = S0(**_kw(), return_hits=3, hits_grad=True, absgrad=True, return_picks=True, return_distortion=True)
    assert both.hits_grad and both.absgrad and both.return_picks and both.return_distortion and both.return_hits == 3
    assert type(S0(**_kw(), return_hits=1, hits_grad=1).hits_grad) is bool


def test_hits_grad_without_hit_slots_is_a_value_error():
    S0 = g.GaussianRasterizationSettings
    with pytest.raises(ValueError, match="hits_grad"):
        S0(**_kw(), hits_grad=True)
    with pytest.raises(ValueError, match="hits_grad"):
        S0(**_kw(), return_hits=0, hits_grad=True)
    with pytest.raises(ValueError, match="hits_grad"):
        S0(**_kw())._replace(hits_grad=True)
    with pytest.raises(ValueError, match="hits_grad"):
        S0(**_kw(), return_hits=4, hits_grad=True)._replace(return_hits=0)
    with pytest.raises(ValueError, match="return_hits"):
        S0(**_kw(), return_hits=33, hits_grad=True)
    S0(**_kw(), hits_grad=False)   # off needs nothing


def test_call_site_keywords():
    for fn in (S.render_cuda, S.render_color_and_depth, S.render_views_fused, S.DecoderSplattingCUDA.forward, S.boundary_arguments):
        p = inspect.signature(fn).parameters
        assert "hits_grad" in p and p["hits_grad"].default is False and p["hits_grad"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        names = list(p)   # (where return_hits was placed: in front of the older keyword-only flags, no positional parameter moved)
        assert names[-4:] == ["hits_grad", "return_hits", "return_picks", "return_contributions"]


def test_boundary_arguments_passes_the_flag_on_and_refuses_it_without_slots():
    b, gN = 1, 5
    ext = torch.eye(4)[None]
    K = torch.tensor([[[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1]]])
    near, far = torch.tensor([0.5]), torch.tensor([50.0])
    args = (ext, K, near, far, (8, 8), torch.zeros(b, 3), torch.rand(b, gN, 3), torch.eye(3).expand(b, gN, 3, 3) * 0.01,
            torch.rand(b, gN, 3, 1), torch.rand(b, gN))
    (rs, _kw2), = S.boundary_arguments(*args, return_hits=3, hits_grad=True)
    assert rs.return_hits == 3 and rs.hits_grad is True
    (rs, _kw2), = S.boundary_arguments(*args, return_hits=3)
    assert rs.return_hits == 3 and rs.hits_grad is False
    (rs, _kw2), = S.boundary_arguments(*args)
    assert rs.return_hits == 0 and rs.hits_grad is False
    with pytest.raises(ValueError, match="hits_grad"):
        S.boundary_arguments(*args, hits_grad=True)


def test_composite_hits_is_differentiable_in_weights_that_carry_a_graph():
    """what `hits_grad` makes of composite_hits: with weights that require grad, the composite's gradient reaches them"""
    idx = torch.tensor([[[0, 2]], [[1, -1]]], dtype=torch.int32)             # K = 2, 1 × 2 pixels
    w = torch.tensor([[[0.5, 0.25]], [[0.125, 0.0]]], requires_grad=True)
    vals = torch.tensor([1.0, 2.0, 4.0], requires_grad=True)
    hits = g.PixelHits(idx, w, torch.zeros(1, 2), torch.tensor([[2, 1]], dtype=torch.int32))
    out = g.composite_hits(vals, hits)
    assert torch.allclose(out, torch.tensor([[0.5 * 1 + 0.125 * 2, 0.25 * 4]]))
    out.sum().backward()
    assert torch.equal(w.grad, torch.tensor([[[1.0, 4.0]], [[2.0, 0.0]]]))   # values[index], 0 at the padding slot
    assert torch.equal(vals.grad, torch.tensor([0.5, 0.125, 0.25]))
