"""tests/golden/epipolar_*.npz (made by tests/golden/make_epipolar_golden.py from the reference's own sampler): the files hold
the documented keys with consistent shapes and dtypes, both precisions, and their recorded inputs obey the margin rule of
tests/epipolar_reference.py — so that `valid` can be demanded equal on every ray."""
import numpy as np
import pytest

from tests.epipolar_reference import margin_violations
from tests.test_epipolar_reference import NAMES, load_golden

PER_SAMPLE = {"features": None, "xy_sample": 2, "xy_sample_near": 2, "xy_sample_far": 2, "depth": 0, "raw_depth": 0}


@pytest.mark.parametrize("name", NAMES)
def test_keys_shapes_and_the_margin_rule(name):
    case, z = load_golden(name)
    b, v, c, h, w = case["images"].shape
    s, win = case["num_samples"], case["ray_window"]
    r = h * w if win is None else (win[1] - win[0]) * (win[3] - win[2])
    assert (name == "window") == (win is not None)
    assert z["extrinsics"].shape == (b, v, 4, 4) and z["intrinsics"].shape == (b, v, 3, 3) and z["near"].shape == z["far"].shape == (b, v)
    assert z["valid"].dtype == np.bool_ and z["valid"].shape == (b, v, v - 1, r)
    for tag, dtype in (("32", np.float32), ("64", np.float64)):
        for k, tail in PER_SAMPLE.items():
            shape = (b, v, v - 1, r, s) + ((c,) if tail is None else (tail,) if tail else ())
            assert z[k + tag].dtype == dtype and z[k + tag].shape == shape, (k, tag)
        assert z["origins" + tag].shape == z["directions" + tag].shape == (b, v, r, 3)
        assert z["xy_ray" + tag].shape == (b, v, h * w, 2)      # (the reference does not crop xy_ray)
        assert np.isfinite(z["features" + tag]).all() and np.isfinite(z["depth" + tag]).all()
    assert set(z.files) == ({"images", "extrinsics", "intrinsics", "near", "far", "num_samples", "seed", "ray_window", "valid"} |
                            {k + t for k in list(PER_SAMPLE) + ["origins", "directions", "xy_ray"] for t in ("32", "64")})
    assert margin_violations(case) == 0
    assert s & (s - 1) == 0      # (a power of two: the reference's float32 sample positions are exact in its float64 run)
