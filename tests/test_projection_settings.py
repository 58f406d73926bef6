"""`return_projection` in GaussianRasterizationSettings — no GPU: the setting is kept beside the tuple exactly as `return_hits`
is (construction, `_replace`, `_asdict`, `__repr__`), the tuple's items are unchanged, and anything truthy is coerced to bool."""
import pytest
import torch

from ggrt_official_amd import GaussianRasterizationSettings, Projection
from ggrt_official_amd.rasterizer import _RasterizationSettingsFields as S0, _with_contributions


def _settings(**kw):
    return GaussianRasterizationSettings(image_height=4, image_width=6, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                         scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                         campos=torch.zeros(3), prefiltered=False, **kw)


def test_default_is_off_and_the_keyword_turns_it_on():
    assert _settings().return_projection is False and GaussianRasterizationSettings.return_projection is False
    assert _settings(return_projection=True).return_projection is True


def test_keyword_only():
    n = len(S0._fields)
    args = tuple(_settings())
    assert len(args) == n
    with pytest.raises(TypeError):
        GaussianRasterizationSettings(*args, False, False, True)   # behind return_contributions / return_picks: no third slot
    assert GaussianRasterizationSettings(*args, return_projection=True).return_projection is True


def test_replace_asdict_repr_carry_it():
    on, off = _settings(return_projection=True), _settings()
    assert on._replace(image_height=8).return_projection is True and on._replace(image_height=8).image_height == 8
    assert on._replace(return_projection=False).return_projection is False
    assert off._replace(return_projection=True).return_projection is True
    both = on._replace(return_hits=4, hits_grad=True, absgrad=True)
    assert both.return_projection is True and both.return_hits == 4 and both.hits_grad and both.absgrad
    assert on._asdict()["return_projection"] is True and off._asdict()["return_projection"] is False
    assert list(on._asdict())[:len(S0._fields)] == list(S0._fields)
    assert "return_projection=True" in repr(on) and "return_projection=False" in repr(off)


def test_tuple_items_unchanged():
    on, off = _settings(return_projection=True), _settings()
    assert on._fields == off._fields == S0._fields and "return_projection" not in on._fields
    assert len(on) == len(off) == len(S0._fields)
    assert all(a is b or a == b for a, b in zip(list(on)[:4], list(off)[:4]))
    assert GaussianRasterizationSettings._make(tuple(on)).return_projection is False   # (the bare items do not carry it)


@pytest.mark.parametrize("value,want", [(1, True), (0, False), ("yes", True), (None, False), ([], False)])
def test_bool_coercion(value, want):
    assert _settings(return_projection=value).return_projection is want
    assert _settings()._replace(return_projection=value).return_projection is want


def test_the_public_tuple_ends_in_one_projection_element():
    raw = tuple(range(3)) + tuple("abcd") + tuple("uvwxyz")   # colour, radii, depth | hits | projection
    out = _with_contributions(raw, False, False, True, True)
    assert len(out) == 5 and isinstance(out[-1], Projection) and tuple(out[-1]) == tuple("uvwxyz")
    assert tuple(out[-2]) == tuple("abcd") and out[:3] == (0, 1, 2)
    assert Projection._fields == ("means2d", "depth", "conic", "opacity", "color", "valid")
    assert _with_contributions(raw[:3], False) == raw[:3]
    import diff_gaussian_rasterization as shim
    assert shim.Projection is Projection
