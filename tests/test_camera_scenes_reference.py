"""The two references on the scenes of tests/camera_scenes.py, WITHOUT a GPU: before a kernel is held to them off the
synthetic camera family (tests/test_gpu_camera_family.py), `oracle/ggr_oracle.c` and `oracle/torch_raster.py` are proven
against each other there — beyond the frustum clamp, around the near cull, with scale_modifier ≠ 1, quaternions that are not
unit, an off-centre principal point, non-square pixels and 25° / 100° fields of view.  Every constructor's own property
assertion runs inside (a scene that missed its target fails here, not silently).

Bars: discrete outputs equal; image and gradients within the strict bars of tests/helpers.py with nothing set aside
(measured: images ≤ 1.7e-6, gradients ≤ 5e-6 rel-L2 between the C oracle and fp32 torch autograd)."""
import numpy as np
import pytest
import torch

from ggrt_official_amd.synthetic import camera_matrices, upstream_gradient
from oracle import c_oracle
from tests import camera_scenes as C
from tests.helpers import FWD_ATOL, check_grads, check_image, rel_l2

SMALL = dict(clamp=dict(P=1500, W=80, H=64), near=dict(P=1500, W=80, H=64), on_cull=dict(P=1500, W=80, H=64),
             camera=dict(P=1500, W=86, H=68, fov_deg=25.0, cx=0.6, cy=0.45, aspect=0.8), modifier=dict(P=1500, W=80, H=64),
             mixed=dict(P=1500, W=86, H=68))
KEYS = ["means3D", "opacities", "shs", "scales", "rotations"]


def _scene(name):
    return C.CONSTRUCTORS[name](seed=0, **SMALL[name])


def _against_the_c_oracle(cs, dtype):
    dL = upstream_gradient(cs.sc.width, cs.sc.height, seed=3)
    st = C.oracle_state(cs, tight=False)                      # the reference's rects: what the torch leg bins by
    ref = c_oracle.backward(st, dL.numpy())
    t = C.torch_run(cs, dL, dtype=dtype)
    assert np.array_equal(t["radii"], st.radii)
    assert t["num_rendered"] == st.num_rendered
    assert np.array_equal(t["point_list"].astype(np.uint32), st.point_list)
    assert np.array_equal(t["ranges"], st.ranges)
    check_image(t["color"], st.color, tag=f"camera_scenes:{cs.name}:{dtype}")
    assert np.abs(t["color"] - st.color).max() <= FWD_ATOL       # (no threshold flip on these seeds: every pixel)
    check_grads(t["grads"], ref, KEYS, tag=f"camera_scenes:{cs.name}:{dtype}")
    return st, t


@pytest.mark.parametrize("name", list(C.CONSTRUCTORS))
def test_c_oracle_equals_fp32_torch_autograd(name):
    _against_the_c_oracle(_scene(name), torch.float32)


@pytest.mark.parametrize("name", [n for n in C.CONSTRUCTORS if n != "on_cull"])   # (float32 0.2 read as a double is > 0.2)
def test_c_oracle_against_fp64_torch_autograd(name):
    _against_the_c_oracle(_scene(name), torch.float64)


@pytest.mark.parametrize("name", list(C.POSE_CASES))
def test_camera_gradient_cases_are_flip_free_and_their_spread_is_as_recorded(name):
    """fp32 against fp64 torch autograd on the GPU file's camera-gradient cases: the same discrete decisions, and the spread
    the GPU bars are 10 × of (camera_scenes.POSE_CASES) is not understated."""
    case = C.POSE_CASES[name]
    cs = case["make"]()
    dL, dLd, sel = C.pose_gradients(cs, case)
    a = C.torch_run(cs, dL, dLd, torch.float32, pose=True, tile_filter=sel)
    b = C.torch_run(cs, dL, dLd, torch.float64, pose=True, tile_filter=sel)
    assert C.flip_free(a, b, FWD_ATOL, order=case.get("order", True))
    for k, recorded in case["spread"].items():
        r = rel_l2(a["grads"][k], b["grads"][k])
        print(f"{name} {k}: fp32 vs fp64 rel-L2 {r:.2e} (recorded {recorded:.2e})")
        assert r <= 1.5 * recorded, (k, r, recorded)      # (thread counts move the last digits of a sum; not the order)


def test_launch_set_views_are_flip_free_and_their_spread_is_as_recorded():
    cs, views = C.launch_set()
    assert len({v.sc.tanfovx for v in views}) == len(views)
    for v, cv in enumerate(views):
        dL = upstream_gradient(cv.sc.width, cv.sc.height, seed=20 + v)
        a = C.torch_run(cv, dL, None, torch.float32, pose=True)
        b = C.torch_run(cv, dL, None, torch.float64, pose=True)
        assert C.flip_free(a, b, FWD_ATOL), v
        for k, recorded in zip(("viewmatrix", "projmatrix", "campos"), C.LAUNCH_SET_SPREAD[v]):
            r = rel_l2(a["grads"][k], b["grads"][k])
            print(f"view {v} {k}: fp32 vs fp64 rel-L2 {r:.2e} (recorded {recorded:.2e})")
            assert r <= 1.5 * recorded, (v, k, r, recorded)


def test_square_pixels_reproduce_camera_matrices():
    pose = C.pose(4)
    view, full, campos, tx, ty = C.camera(100, 60, 60.0, 1.0, 0.4, 0.6, pose)
    v0, f0, c0, tx0, ty0, _, _ = camera_matrices(100, 60, 60.0, c2w=pose, cx=0.4, cy=0.6)
    assert torch.equal(view, v0) and torch.equal(full, f0) and abs(tx - tx0) < 1e-7 and abs(ty - ty0) < 1e-7
    _, f1, _, _, ty1 = C.camera(100, 60, 60.0, 1.0 + 1e-12, 0.4, 0.6, pose)      # the module's own projection, same camera
    assert torch.allclose(f1, f0, rtol=1e-6, atol=1e-7)


# ---- identities the formulas imply ------------------------------------------------------------------------------------------------
def _with(cs, scale_modifier=None, scales=None):
    out = C.copy_scene(cs) if scales is None else C.copy_scene(cs, scales=scales)
    out.scale_modifier = cs.scale_modifier if scale_modifier is None else scale_modifier
    return out


STATE = ("radii", "tiles_touched", "depth", "xy", "conic_opacity", "rgb", "cov3D", "point_list", "ranges", "color", "final_T")


@pytest.mark.parametrize("m", [0.5, 2.0, 1.7])
def test_scale_modifier_is_a_factor_on_the_scales(m):
    """scale_modifier = m with scales s renders what scale_modifier = 1 with scales m·s renders: bit for bit when m is a power
    of two, within rounding otherwise; d/ds is m times the gradient w.r.t. the scaled scales."""
    cs = _scene("modifier")
    dL = upstream_gradient(cs.sc.width, cs.sc.height, seed=3)
    a = C.oracle_state(_with(cs, scale_modifier=m))
    b = C.oracle_state(_with(cs, scale_modifier=1.0, scales=cs.sc.scales * m))
    ga, gb = c_oracle.backward(a, dL.numpy()), c_oracle.backward(b, dL.numpy())
    if m in (0.5, 2.0):
        for k in STATE:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert np.array_equal(ga["scales"], np.float32(m) * gb["scales"])
        for k in ("means3D", "opacities", "shs", "rotations"):
            assert np.array_equal(ga[k], gb[k]), k
    else:
        assert (a.radii != b.radii).mean() < 1e-3                 # (a radius is a ceil: one in thousands may sit on an integer)
        check_image(a.color, b.color)
        check_grads({**ga, "scales": ga["scales"] / m}, gb, KEYS)


def test_cov3d_precomp_ignores_scale_modifier():
    cs = _scene("modifier")
    dL = upstream_gradient(cs.sc.width, cs.sc.height, seed=3)
    a = C.oracle_state(_with(cs, scale_modifier=1.7), use_cov=True)
    b = C.oracle_state(_with(cs, scale_modifier=1.0), use_cov=True)
    for k in STATE:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    ga, gb = c_oracle.backward(a, dL.numpy()), c_oracle.backward(b, dL.numpy())
    for k in ("means3D", "opacities", "shs", "cov3D_precomp"):
        assert np.array_equal(ga[k], gb[k]), k
    ta = C.torch_run(_with(cs, scale_modifier=1.7), dL, use_cov=True)
    tb = C.torch_run(_with(cs, scale_modifier=1.0), dL, use_cov=True)
    assert np.array_equal(ta["color"], tb["color"]) and np.array_equal(ta["grads"]["cov3D_precomp"], tb["grads"]["cov3D_precomp"])
    # and it is the same scene as the scale + rotation form WITH the modifier (cov3D holds modifier·scale)
    c = C.oracle_state(cs)
    assert (c.radii != a.radii).mean() < 1e-3
    check_image(a.color, c.color)


def test_a_clamped_mean_moves_on_screen_but_keeps_its_conic():
    """The clamp's rule is straight-through, so a finite difference does not apply to the clamped coordinate.  What holds
    instead: moving a clamped Gaussian further out along its clamped axis leaves the Jacobian — hence the conic and the
    radius — exactly what it was, while its screen position moves."""
    cs = _scene("clamp")                                          # identity pose: the camera's axes are the world's
    st = C.oracle_state(cs)
    cls, _, _ = C.clamp_classes(cs, st)
    for k, axes in (("x_only", [0]), ("y_only", [1]), ("both", [0, 1])):
        ids = np.flatnonzero(cls[k])
        moved = C.copy_scene(cs)
        for a in axes:
            moved.sc.means3D[ids, a] *= 1.0625
        st2 = C.oracle_state(moved)
        both = ids[(st2.radii[ids] > 0)]
        assert len(both) >= 10, (k, len(both))
        assert np.array_equal(st2.conic_opacity[both], st.conic_opacity[both]), k
        assert np.array_equal(st2.radii[both], st.radii[both]), k
        for a in axes:
            assert (np.abs(st2.xy[both, a] - st.xy[both, a]) > 1.0).all(), k
        other = [a for a in (0, 1) if a not in axes]
        assert np.array_equal(st2.xy[both][:, other], st.xy[both][:, other])
    # an unclamped Gaussian's conic does move with its mean
    inside = np.flatnonzero((st.radii > 0) & ~cs.groups["clamp"])[:50]
    moved = C.copy_scene(cs)
    moved.sc.means3D[inside, 0] *= 1.0625
    st3 = C.oracle_state(moved)
    seen = inside[st3.radii[inside] > 0]
    assert (st3.conic_opacity[seen, :3] != st.conic_opacity[seen, :3]).any(1).mean() > 0.9


def test_both_fp32_references_cull_at_and_below_the_near_plane():
    cs = _scene("on_cull")
    st = C.oracle_state(cs, tight=False)
    t = C.torch_run(cs, upstream_gradient(cs.sc.width, cs.sc.height, seed=3), dtype=torch.float32)
    g = cs.groups
    for radii in (st.radii, t["radii"]):
        assert not radii[g["at_cull"]].any() and not radii[g["below_cull"]].any()
        assert (radii[g["above_cull"]] > 0).mean() > 0.9
    assert np.array_equal(st.radii, t["radii"])
    for k in KEYS:                                                # a culled Gaussian has no gradient
        assert not np.any(t["grads"][k][g["at_cull"] | g["below_cull"]]), k
