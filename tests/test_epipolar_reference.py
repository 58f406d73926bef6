"""The torch restatement of the epipolar sampling stage (tests/epipolar_reference.py) against fixtures recorded from the
reference's own `EpipolarSampler.forward` + `get_depth` + clip + `depth_to_relative_disparity` (tests/golden/epipolar_*.npz,
made by tests/golden/make_epipolar_golden.py), in float64, and against finite differences."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.epipolar_reference import FLOAT_OUTPUTS, epipolar_reference, make_case, run_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("apart", "three_views", "two_views", "window")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, f"epipolar_{name}.npz"), allow_pickle=False)
    case = {k: torch.from_numpy(z[k]) for k in ("images", "extrinsics", "intrinsics", "near", "far")}
    case["num_samples"] = int(z["num_samples"])
    case["ray_window"] = tuple(int(q) for q in z["ray_window"]) or None
    return case, z


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def test_the_fixtures_are_all_here():
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "epipolar_*.npz"))) == [f"epipolar_{n}.npz" for n in NAMES]


@pytest.mark.parametrize("name", NAMES)
def test_the_float64_restatement_reproduces_the_reference(name):
    """`valid` equal on every ray; every float output within 1e-9 relative of the reference's float64 run.  The depth differs by
    what the closed-form solve makes against the reference's torch.linalg.lstsq — measured on these four fixtures: at most
    7.9e-14 (relative disparity) and 5.4e-13 (clipped depth), relative to the largest value; the bars are ten times that.
    With a ray window the reference returns xy_ray for the WHOLE grid (it crops origins and directions only); the restatement
    returns the window's rays, which are compared with the window's rows of the reference's."""
    case, z = load_golden(name)
    out = run_case(epipolar_reference, case, details=True)
    assert np.array_equal(out["valid"].numpy(), z["valid"])
    b, v, c, h, w = case["images"].shape
    for k in FLOAT_OUTPUTS + ("raw_depth",):
        want = torch.from_numpy(z[k + "64"])
        if k == "xy_ray" and case["ray_window"] is not None:
            y0, y1, x0, x1 = case["ray_window"]
            want = want.reshape(b, v, h, w, 2)[:, :, y0:y1, x0:x1].reshape(b, v, -1, 2)
        assert want.dtype == torch.float64 and out[k].shape == want.shape, k
        bar = {"depth": 7.9e-13, "raw_depth": 5.4e-12}.get(k, 1e-9)
        assert _rel(out[k], want) <= bar, (k, _rel(out[k], want))
    if name == "apart":
        assert not z["valid"].any() and float(out["features"].abs().max()) == 0
    else:
        assert z["valid"].mean() > 0.5


def test_the_float32_restatement_errs_like_the_references_float32_run():
    """the float32 torch route that sets the GPU tests' bar is no worse than three times the reference's own float32 run"""
    for name in ("two_views", "three_views", "window"):
        case, z = load_golden(name)
        low = run_case(epipolar_reference, case, dtype=torch.float32)
        assert np.array_equal(low["valid"].numpy(), z["valid"])
        for k in ("features", "xy_sample", "depth"):
            want = torch.from_numpy(z[k + "64"])
            own, theirs = _rel(low[k].double(), want), _rel(torch.from_numpy(z[k + "32"]).double(), want)
            assert own <= max(3 * theirs, 1e-6), (name, k, own, theirs)


def test_gradcheck_of_features_with_respect_to_the_feature_maps():
    case = make_case(1, 2, 3, 4, 2, 4, 11)
    images = case["images"].clone().requires_grad_(True)
    fn = lambda im: run_case(epipolar_reference, dict(case, images=im))["features"]
    assert bool(run_case(epipolar_reference, case)["valid"].any())
    assert torch.autograd.gradcheck(fn, (images,), eps=1e-6, atol=1e-8)


def test_all_four_branches_of_project_rays_occur_in_the_case_families():
    """(min_valid, max_valid): which of the near / far projections fall inside the other frame"""
    counts = {(a, b): 0 for a in (True, False) for b in (True, False)}
    for family, v in (("default", 3), ("inside", 2), ("clipped", 2), ("nearfar", 2)):
        out = run_case(epipolar_reference, make_case(1, v, 11, 13, 1, 8, 21, family), details=True)
        for key in counts:
            counts[key] += int(((out["min_valid"] == key[0]) & (out["max_valid"] == key[1])).sum())
    assert all(n > 0 for n in counts.values()), counts
