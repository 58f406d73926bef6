"""Where the reference is present (the build container), tests/golden/warp_cost_*.npz must be exactly what
tests/golden/make_warp_cost_golden.py produces from it: the fixtures ARE outputs of the reference's own `DepthPoseNet.get_cost_each`
and `depth_cost_calc`, not hand-edited arrays.  Skipped where the reference does not exist; the generator runs in a subprocess (it
injects stub modules and, for its float64 run, patches `torch.Tensor.float`)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/ggrt"), reason="the reference tree is not on this machine")


def test_warp_cost_fixtures_are_what_the_generator_produces(tmp_path):
    env = dict(os.environ, GGR_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS="4")
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_warp_cost_golden.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "warp_cost_*.npz")))
    assert len(names) == 4 and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(tmp_path), "warp_cost_*.npz")))
    for n in names:
        a, b = np.load(os.path.join(GOLDEN, n), allow_pickle=False), np.load(os.path.join(str(tmp_path), n), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), n
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (n, k)
            if k.endswith("32"):   # (a thread count may change a summation order inside the float32 sums)
                np.testing.assert_allclose(a[k], b[k], rtol=0, atol=2e-6, err_msg=f"{n}:{k}")
            elif k.endswith("64"):
                np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-13, err_msg=f"{n}:{k}")
            else:                  # inputs and settings: to the bit
                assert np.array_equal(a[k], b[k]), (n, k)
