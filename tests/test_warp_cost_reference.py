"""The torch restatement of the feature-metric cost map (tests/warp_cost_reference.py) against fixtures made by the reference's own
`DepthPoseNet.get_cost_each` / `depth_cost_calc` (tests/golden/make_warp_cost_golden.py): in float64 it equals them to 1e-12, cost and
all four gradients, in both forms; it passes gradcheck away from cell borders; and `decisions` taken from its own floors change
nothing.  Also the conditions the GPU tests put on their inputs, checked here for the float64 restatement alone."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.warp_cost_reference import INPUTS, make_warp_case, near_border_share, run_warp_cost, warp_cost_reference

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
}
FULL_CASE = (5, 128, 48, 63, 821, 1.0 / 8)


def _load(name):
    z = np.load(os.path.join(GOLDEN, f"warp_cost_{name}.npz"), allow_pickle=False)
    case = {k: torch.from_numpy(z[k]) for k in INPUTS + ("K", "ref_Ks", "g_mean", "g_none")}
    return z, case


def test_there_are_three_fixtures_of_tens_of_kilobytes():
    assert len(FIXTURES) == 3
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


@pytest.mark.parametrize("opts", [dict(scale_factor=1.0 / 8), dict(scale_factor=1.0, disp_range=(1.0, 100.0))])
@pytest.mark.parametrize("form", ["none", "mean"])
def test_gradcheck_away_from_cell_borders(form, opts):
    case = make_warp_case(2, 2, 4, 5, 830, scale_factor=opts["scale_factor"], disp_range=opts.get("disp_range"))
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
