"""The torch restatement of the feature-metric cost map (tests/warp_cost_reference.py) against fixtures made by the reference's own
`DepthPoseNet.get_cost_each` / `depth_cost_calc` (tests/golden/make_warp_cost_golden.py): in float64 it equals them to 1e-12, cost and
all four gradients, in both forms; it passes gradcheck away from cell borders; and `decisions` taken from its own floors change
nothing.  Also the conditions the GPU tests put on their inputs, checked here for the float64 restatement alone."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.warp_cost_reference import (DEPTH_COLUMN_VALUES, INPUTS, LARGE_ANGLES, depth_class, folded32, frame_masks, make_warp_case, near_border_share,
                                       run_warp_cost, warp_cost_reference)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f)[len("warp_cost_"):-4] for f in glob.glob(os.path.join(GOLDEN, "warp_cost_*.npz")))

TP, G, CS = 64, 8, 32          # kWarpTilePixels, kWarpGroups, kWarpChannelSlice of csrc/warp_cost.h
# name: (V, C, h, w, seed, scale_factor, reduce, make_warp_case options) — the GPU tests' shapes: the pixel tile's edge (63, 64, 65
# pixels; two tiles and one pixel), the wave split's (C = 7, 8, 9) and the channel slice's (31, 32, 33, two slices and one), 2 x 2,
# C in {1, 3, 33, 128}, V in {1, 2, 5}, both reduce forms, both scale factors, K != ref_K throughout, the folded disparity on and off
GPU_CASES = {
    "px63_c7": (2, 7, 7, 9, 810, 1.0 / 8, "mean", {}),
    "px64_c8": (2, 8, 8, 8, 811, 1.0, "none", {}),
    "px65_c9": (1, 9, 5, 13, 812, 1.0 / 8, "none", dict(disp_range=(1.0, 100.0))),
    "px129_c31": (2, 31, 3, 43, 813, 1.0, "mean", dict(disp_range=(1.0, 100.0))),
    "px128_c32": (1, 32, 8, 16, 814, 1.0 / 8, "mean", {}),
    "c33_v5": (5, 33, 6, 11, 815, 1.0 / 8, "none", {}),
    "c65": (2, 65, 4, 5, 816, 1.0, "none", {}),
    "tiny_2x2_c1": (1, 1, 2, 2, 817, 1.0 / 8, "mean", {}),
    "c3_v5_mean": (5, 3, 9, 12, 818, 1.0, "mean", {}),
    "c128_small": (2, 128, 5, 6, 819, 1.0 / 8, "mean", {}),
    "nonpositive_block": (2, 3, 9, 12, 820, 1.0 / 8, "mean", dict(nonpositive_block=True)),
    # loop trips that run a second time: tile_coordinates' over view x pixel (V > 8; V = 16 is the cap) and the pose kernel's over
    # the tiles (more than 64); Euler angles of tenths of a radian; a view whose P.z changes sign inside a tile; a column of inverse
    # depths on both sides of the 1e-6 gate (folded: a disp_range whose fold float32 evaluates exactly, see _raw_disparity)
    "v9_mean": (9, 3, 5, 13, 850, 1.0 / 8, "mean", {}),
    "v16_none": (16, 2, 9, 8, 851, 1.0, "none", {}),
    "v16_mean_c33": (16, 33, 4, 17, 852, 1.0 / 8, "mean", dict(disp_range=(1.0, 100.0))),
    "tiles65": (2, 2, 65, 64, 853, 1.0, "mean", {}),
    "tiles130_tail": (2, 1, 43, 193, 854, 1.0 / 8, "none", {}),
    "large_angles": (3, 5, 9, 12, 855, 1.0 / 8, "none", dict(angles=LARGE_ANGLES)),
    "large_angles_mean": (3, 9, 7, 19, 856, 1.0, "mean", dict(angles=LARGE_ANGLES, disp_range=(1.0, 100.0))),
    "straddle": (2, 3, 9, 12, 857, 1.0 / 8, "none", dict(straddle_view=0)),
    "depth_column": (2, 3, 6, 11, 858, 1.0 / 8, "mean", dict(depth_column=5)),
    "depth_column_disp": (2, 3, 6, 11, 859, 1.0, "none", dict(depth_column=5, disp_range=(1.0, 128.0))),
}
COLLAPSE_CASE = (1, 2, 8, 16, 860, 1.0)          # V, C, h, w, seed, scale_factor of test_scatter_into_one_cell
FULL_CASE = (5, 128, 48, 63, 821, 1.0 / 8)


def _load(name):
    z = np.load(os.path.join(GOLDEN, f"warp_cost_{name}.npz"), allow_pickle=False)
    case = {k: torch.from_numpy(z[k]) for k in INPUTS + ("K", "ref_Ks", "g_mean", "g_none")}
    return z, case


def test_there_are_four_fixtures_of_tens_of_kilobytes():
    assert len(FIXTURES) == 4
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f"warp_cost_{n}.npz")) < 100 * 1024
    z, _ = _load("v3c5_unit_far")
    assert float(z["scale_factor"]) == 1.0
    z2, case = _load("v3c5_unit_far")
    ref = run_warp_cost("torch", case, torch.float64, "cpu", reduce="none", scale_factor=1.0)
    u = ref["coords"][1, 0]
    out = float(((u <= -1) | (u >= 7)).double().mean())
    assert 0.1 < out < 0.9, out                 # one view partly out of frame
    assert _load("v1c1_tiny")[1]["fmap"].shape == (1, 1, 2, 2) and _load("v2c3_eighth")[1]["fmaps_ref"].shape == (2, 3, 9, 12)
    z, case = _load("v2c3_large_angles")
    assert case["fmaps_ref"].shape == (2, 3, 7, 10) and float(z["scale_factor"]) == 1.0 / 8
    assert torch.equal(case["poses"][:, 3:], torch.tensor(LARGE_ANGLES[:2], dtype=torch.float32))


@pytest.mark.parametrize("form", ["none", "mean"])
@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_equals_the_reference(name, form):
    z, case = _load(name)
    got = run_warp_cost("torch", case, torch.float64, "cpu", reduce=form, scale_factor=float(z["scale_factor"]))
    np.testing.assert_allclose(got["cost"].numpy(), z[f"cost_{form}64"], rtol=0, atol=1e-12)
    for k in INPUTS:
        np.testing.assert_allclose(got["g_" + k].numpy(), z[f"g_{k}_{form}64"], rtol=0, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_restatement_is_close_to_the_reference_in_float32(name):
    z, case = _load(name)
    got = run_warp_cost("torch", case, torch.float32, "cpu", reduce="mean", scale_factor=float(z["scale_factor"]))
    np.testing.assert_allclose(got["cost"].numpy(), z["cost_mean32"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", FIXTURES)
def test_decisions_taken_from_its_own_floors_change_nothing(name):
    z, case = _load(name)
    s = float(z["scale_factor"])
    for form in ("none", "mean"):
        a = run_warp_cost("torch", case, torch.float64, "cpu", reduce=form, scale_factor=s)
        b = run_warp_cost("torch", case, torch.float64, "cpu", reduce=form, scale_factor=s, decisions=a["cells"])
        assert torch.equal(a["cells"], b["cells"])
        assert float((a["cost"] - b["cost"]).abs().max()) <= 1e-15
        for k in INPUTS:
            assert float((a["g_" + k] - b["g_" + k]).abs().max()) <= 1e-13 * max(1.0, float(a["g_" + k].abs().max())), k


def test_decisions_of_a_neighbouring_cell_change_the_value_by_rounding_only():
    """u = 3 sampled as the right end of cell 2 or the left end of cell 3 is the same number."""
    ref = torch.arange(24, dtype=torch.float64).reshape(1, 4, 6) ** 1.5
    from tests.warp_cost_reference import bilinear
    u, v = torch.full((4, 6), 3.0, dtype=torch.float64), torch.full((4, 6), 1.25, dtype=torch.float64)
    a = bilinear(ref, u, v, (torch.full((4, 6), 3), torch.full((4, 6), 1)))
    b = bilinear(ref, u, v, (torch.full((4, 6), 2), torch.full((4, 6), 1)))
    assert float((a - b).abs().max()) <= 1e-13 and float((a - bilinear(ref, u, v)).abs().max()) == 0.0


@pytest.mark.parametrize("opts", [dict(scale_factor=1.0 / 8), dict(scale_factor=1.0, disp_range=(1.0, 100.0)),
                                  dict(scale_factor=1.0 / 8, angles=LARGE_ANGLES[:2])])
@pytest.mark.parametrize("form", ["none", "mean"])
def test_gradcheck_away_from_cell_borders(form, opts):
    opts = dict(opts)
    case = make_warp_case(2, 2, 4, 5, 830, scale_factor=opts["scale_factor"], disp_range=opts.get("disp_range"), angles=opts.pop("angles", None))
    t = {k: v.clone().requires_grad_(k in INPUTS) for k, v in case.items()}
    base = warp_cost_reference(t["fmap"], t["fmaps_ref"], t["inv_depth"], t["K"], t["ref_Ks"], t["poses"], reduce=form, **opts)
    c = base["coords"]
    assert float((c - c.round()).abs().min()) > 1e-3          # no coordinate near a cell border: the function is smooth around the inputs
    fn = lambda f, r, d, p: warp_cost_reference(f, r, d, t["K"], t["ref_Ks"], p, reduce=form, **opts)["cost"]
    assert torch.autograd.gradcheck(fn, (t["fmap"], t["fmaps_ref"], t["inv_depth"], t["poses"]), eps=1e-7, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_keep_away_from_cell_borders(name):
    """The condition the GPU tests put on their inputs, for the float64 restatement alone (float32 on the CPU measures the
    coordinate error): under 2 % of the (view, pixel) pairs within 8 x that error of a border."""
    V, C, h, w, seed, s, form, opts = GPU_CASES[name]
    case = make_warp_case(V, min(C, 2), h, w, seed, scale_factor=s, **opts)
    kw = dict(reduce=form, scale_factor=s, disp_range=opts.get("disp_range"))
    r64 = run_warp_cost("torch", case, torch.float64, "cpu", need=(), **kw)
    r32 = run_warp_cost("torch", case, torch.float32, "cpu", need=(), **kw)
    share, e, ez = near_border_share(r64, r32, h, w)
    print(f"{name}: coordinate error {e:.3e}, P.z error {ez:.3e}, near-border share {share:.4%}")
    assert share < 0.02 and e < 1e-3


def _float64_run(name, need=INPUTS):
    V, C, h, w, seed, s, form, opts = GPU_CASES[name]
    case = make_warp_case(V, min(C, 2), h, w, seed, scale_factor=s, **opts)
    return case, run_warp_cost("torch", case, torch.float64, "cpu", need=need, reduce=form, scale_factor=s, disp_range=opts.get("disp_range"))


def upstream_beyond_tile_63(case):
    """The case with its upstream gradients zeroed on the flat pixel indices below 64 x 64: only the pose kernel's second and
    later strided trips over the tiles then receive anything."""
    case = dict(case)
    for k in ("g_mean", "g_none"):
        g = case[k].clone()
        g.flatten(2)[..., : TP * 64] = 0
        case[k] = g
    return case


def test_the_new_shapes_reach_the_second_trips():
    """tile_coordinates walks nv x 64 entries with 512 threads; the pose kernel walks the tiles with 64."""
    tiles = lambda n: -(-(GPU_CASES[n][2] * GPU_CASES[n][3]) // TP)
    assert GPU_CASES["v9_mean"][0] * TP == 512 + TP and GPU_CASES["v9_mean"][2] * GPU_CASES["v9_mean"][3] == TP + 1
    assert GPU_CASES["v16_none"][0] == GPU_CASES["v16_mean_c33"][0] == 16 and GPU_CASES["v16_mean_c33"][1] == CS + 1
    assert tiles("tiles65") == 65 and GPU_CASES["tiles65"][2] * GPU_CASES["tiles65"][3] == 65 * TP
    assert tiles("tiles130_tail") == 130 and GPU_CASES["tiles130_tail"][2] * GPU_CASES["tiles130_tail"][3] == 129 * TP + 43
    assert max(tiles(n) for n in GPU_CASES if n not in ("tiles65", "tiles130_tail")) <= 64
    V, C, h, w, seed, s, form, opts = GPU_CASES["tiles130_tail"]
    case = upstream_beyond_tile_63(make_warp_case(V, C, h, w, seed, scale_factor=s, **opts))
    assert float(case["g_none"].flatten(2)[..., : 4096].abs().max()) == 0 and float(case["g_none"].flatten(2)[..., 4096:].min()) >= 0.5
    gp = run_warp_cost("torch", case, torch.float64, "cpu", need=("poses",), reduce=form, scale_factor=s)["g_poses"]
    print("tiles130_tail, upstream beyond tile 63 alone: dL/dposes", gp.tolist())
    assert bool((gp.abs().amax(1) > 0).all())


@pytest.mark.parametrize("name", ["large_angles", "large_angles_mean"])
def test_large_angle_cases_stay_in_frame_and_weigh_every_angle(name):
    h, w = GPU_CASES[name][2:4]
    case, r64 = _float64_run(name)
    assert float(case["poses"][:, 3:].abs().min()) >= 0.25
    live4, band = frame_masks(r64, h, w)
    share4, bands = live4.double().flatten(1).mean(1), band.flatten(1).sum(1)
    gp = r64["g_poses"]
    weight = gp[:, 3:].abs() / gp.abs().max()
    print(f"{name}: all four taps live {[round(x, 3) for x in share4.tolist()]}, pixels in the border band {bands.tolist()}, "
          f"angle components of dL/dposes over its maximum {[[round(x, 3) for x in r] for r in weight.tolist()]}")
    assert float(share4.min()) >= 0.30 and int(bands.min()) >= 1 and float(weight.min()) >= 0.01


def test_straddle_case_has_both_sides_of_the_clamp_inside_tile_0():
    h, w = GPU_CASES["straddle"][2:4]
    case, r64 = _float64_run("straddle", need=())
    live4, _ = frame_masks(r64, h, w)
    behind, front = r64["pz"][0] < 1e-5, (r64["pz"][0] >= 1e-5) & live4[0]
    print(f"straddle: view 0 behind {float(behind.double().mean()):.3f}, in front with four live taps {float(front.double().mean()):.3f}; "
          f"in tile 0: {int(behind.flatten()[:TP].sum())} and {int(front.flatten()[:TP].sum())} pixels")
    assert float(behind.double().mean()) >= 0.10 and float(front.double().mean()) >= 0.10
    assert bool(behind.flatten()[:TP].any()) and bool(front.flatten()[:TP].any())
    assert bool((r64["pz"][1] >= 1e-5).all())          # the other view is an ordinary one


@pytest.mark.parametrize("name", ["v16_none", "v16_mean_c33"])
def test_v16_cases_have_every_view_in_frame_with_a_pose_gradient(name):
    h, w = GPU_CASES[name][2:4]
    case, r64 = _float64_run(name)
    live4, band = frame_masks(r64, h, w)
    in_frame = (live4 | band).flatten(1).sum(1)
    print(f"{name}: pixels in frame per view {in_frame.tolist()}, largest |dL/dposes| per view {[f'{x:.2e}' for x in r64['g_poses'].abs().amax(1).tolist()]}")
    assert r64["g_poses"].shape == (16, 6) and int(in_frame.min()) >= 1 and float(r64["g_poses"].abs().amax(1).min()) > 0


@pytest.mark.parametrize("name", ["depth_column", "depth_column_disp"])
def test_depth_column_cases_hold_both_sides_of_the_gate_alike_in_both_precisions(name):
    """The column's inverse depths are finite, fall on the intended side of 0 and of 1e-6 in float64 and in float32 (after the fold,
    where there is one), a point at depth 0 or 1e-3 still projects into the frame, and the float64 gradient is zero exactly where
    the depth is a constant."""
    V, C, h, w, seed, s, form, opts = GPU_CASES[name]
    x = opts["depth_column"]
    case, r64 = _float64_run(name)
    col = case["inv_depth"][0, 0, :, x]
    assert bool(torch.isfinite(case["inv_depth"]).all()) and h == len(DEPTH_COLUMN_VALUES)
    want = depth_class(torch.tensor(DEPTH_COLUMN_VALUES, dtype=torch.float64))
    if "disp_range" in opts:
        lo, hi = 1.0 / opts["disp_range"][1], 1.0 / opts["disp_range"][0]
        assert torch.equal(col, col.float().double())          # (float32 numbers: every route receives the same raw disparity)
        d64, d32 = lo + (hi - lo) * col, folded32(col, opts["disp_range"])
    else:
        d64, d32 = col, col.float()
        assert col.tolist() == list(DEPTH_COLUMN_VALUES)
    print(f"{name}: d in float64 {d64.tolist()}, in float32 {d32.tolist()}")
    assert torch.equal(depth_class(d64), want) and torch.equal(depth_class(d32), want)          # (float32 against the float32 1e-6, as the kernel)
    assert float(((d32.double() - d64).abs() / d64.abs())[want == 2].max()) <= 2.0 ** -22
    live4, band = frame_masks(r64, h, w)
    assert bool((live4 | band)[:, :, x].all())
    g = r64["g_inv_depth"][0, 0, :, x]
    print(f"{name}: float64 dL/dinv_depth down the column {g.tolist()}")
    assert bool((g[want < 2] == 0).all()) and bool((g[want == 2] != 0).all())


def test_collapse_case_samples_one_interior_cell_with_terms_of_one_sign():
    V, C, h, w, seed, s = COLLAPSE_CASE
    case = make_warp_case(V, C, h, w, seed, scale_factor=s, collapse=True)
    r64 = run_warp_cost("torch", case, torch.float64, "cpu", reduce="none", scale_factor=s)
    r32 = run_warp_cost("torch", case, torch.float32, "cpu", need=(), reduce="none", scale_factor=s)
    share, e, ez = near_border_share(r64, r32, h, w)
    u, v = r64["coords"][0, 0], r64["coords"][0, 1]
    print(f"collapse: u in [{float(u.min()):.5f}, {float(u.max()):.5f}], v in [{float(v.min()):.5f}, {float(v.max()):.5f}], coordinate error {e:.3e}")
    cell = torch.tensor([w // 2, h // 2, 0], dtype=torch.int32)
    assert V == 1 and h * w == 2 * TP and share == 0 and e < 1e-3
    assert bool((r64["cells"] == cell).all()) and bool((r32["cells"] == cell).all())
    assert float((u - (w // 2 + 0.3)).abs().max()) < 0.01 and float((v - (h // 2 + 0.6)).abs().max()) < 0.01
    assert float(case["fmap"].min()) == 2.0 and float(case["fmaps_ref"].max()) < 1.5 and float(case["g_none"].min()) >= 0.5
    g = r64["g_fmaps_ref"][0]
    hit = torch.zeros(h, w, dtype=torch.bool)
    hit[h // 2: h // 2 + 2, w // 2: w // 2 + 2] = True
    assert bool((g[:, hit] < 0).all()) and bool((g[:, ~hit] == 0).all())
