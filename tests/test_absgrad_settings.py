"""The `absgrad` setting — the call surface, no GPU."""
import copy
import pickle

import pytest
import torch

import ggrt_official_amd as g


def _kw():
    e = torch.eye(4)
    return dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=e,
                projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False)


def test_absgrad_rides_beside_the_settings_tuple():
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "absgrad" not in S0._fields
    kw = _kw()
    off, on = S0(**kw), S0(**kw, absgrad=True)
    assert off.absgrad is False and on.absgrad is True
    assert on.return_contributions is False and on.return_picks is False and on.return_distortion is False
    assert len(on) == len(off) == len(S0._fields) and tuple(on)[:4] == tuple(off)[:4] and list(on) is not None
    assert on == off and not (on != off)     # equality is the tuple's: the items alone (here the very same objects)
    assert on._replace(sh_max_degree=4).absgrad is True and on._replace(sh_max_degree=4).sh_max_degree == 4
    assert off._replace(absgrad=True).absgrad is True and off.absgrad is False
    both = on._replace(return_distortion=True, return_picks=True)
    assert both.absgrad is True and both.return_distortion is True and both.return_picks is True
    assert both._replace(absgrad=False).return_distortion is True and both._replace(absgrad=False).absgrad is False
    assert on._asdict()["absgrad"] is True and off._asdict()["absgrad"] is False
    assert list(on._asdict())[:len(S0._fields)] == list(S0._fields)
    assert "absgrad=True" in repr(on) and "absgrad=False" in repr(off)
    assert repr(on).endswith("return_contributions=False, return_picks=False)")
    # keyword only: the positional slots behind the tuple's fields stay return_contributions, return_picks
    assert S0(*off).absgrad is False and S0(*off, True, True).absgrad is False
    with pytest.raises(TypeError):
        S0(*off, False, False, True)
    assert S0._make(list(on)).absgrad is False
    assert copy.copy(on).absgrad is True and pickle.loads(pickle.dumps(on)).absgrad is True


def test_the_import_shim_carries_the_setting():
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(**_kw(), absgrad=True)
    assert dgr.GaussianRasterizer(rs)._settings_for_call().absgrad is True


def test_rasterize_views_without_means2d_raises_naming_the_argument():
    rs = g.GaussianRasterizationSettings(**_kw(), absgrad=True)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="means2D"):
        g.rasterize_views(z, torch.zeros(4, 1), torch.eye(4)[None], torch.eye(4)[None], torch.zeros(1, 3), torch.zeros(1, 3),
                          torch.ones(1, 2), rs, colors_precomp=z, cov3D_precomp=torch.zeros(4, 6))
