"""The projection reference (tests/projection_reference.py) on the CPU: the conditions under which tests/test_gpu_projection.py
may hold the GPU to EQUALITY on `valid`, and under which its scenes exercise what they are meant to."""
import pytest
import torch

from tests import projection_reference as pj

NAMES = list(pj.REF_CASES)


@pytest.mark.parametrize("name", NAMES)
def test_float32_and_float64_agree_on_valid(name):
    a, b = pj.ref_projection(name, torch.float32), pj.ref_projection(name, torch.float64)
    assert a["valid"].dtype == torch.bool and torch.equal(a["valid"], b["valid"])
    for f in pj.FIELDS:   # … and on the values, to float32's precision
        assert a[f].dtype == torch.float32 and b[f].dtype == torch.float64 and a[f].shape == b[f].shape
        assert torch.allclose(a[f].double(), b[f], rtol=1e-3, atol=1e-3), f


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_has_invalid_and_valid_rows(name):
    P = pj.REF_CASES[name][0]
    r = pj.ref_projection(name)
    assert r["valid"].shape == (P + pj.N_EXTRA,)
    assert not bool(r["valid"][P:].any()), "the eight appended rows must be invalid"
    assert int((~r["valid"]).sum()) >= 8 and int(r["valid"].sum()) >= 8
    for f in pj.FIELDS:   # invalid rows hold exactly 0, valid rows are not all 0
        assert not bool(r[f][~r["valid"]].any()) and bool(r[f][r["valid"]].any()), f
    sc, _colors = pj.ref_scene(name)
    z = sc.means3D[P:, 2]
    assert int((z < 0.2).sum()) == 4 and int((z >= 0.2).sum()) == 4   # four behind the near cull, four outside the frustum


@pytest.mark.parametrize("name", [n for n in NAMES if pj.REF_CASES[n][4]])
def test_sh_scenes_have_a_clamped_colour_channel_among_valid_rows(name):
    r = pj.ref_projection(name)
    hit = r["clamped"] & r["valid"][:, None]
    assert bool(hit.any())
    assert not bool(r["color"][hit].any())   # a clamped channel is 0 …
    g = pj.ref_grads(name, dict(color=torch.ones_like(r["color"]).float()))
    assert abs(g["shs"]).max() > 0           # … and the colour loss still reaches the SH rows of the others


def test_a_missing_field_has_no_term_and_invalid_rows_get_no_gradient():
    name = NAMES[2]
    r = pj.ref_projection(name)
    g = pj.ref_grads(name, dict(opacity=torch.ones_like(r["opacity"]).float()))
    assert not g["means3D"].any() and not g["cov3D_precomp"].any() and not g["shs"].any()   # (no anti-aliasing in this scene)
    assert (g["opacities"].reshape(-1) == r["valid"].double().numpy()).all()
