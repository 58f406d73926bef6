"""Where the reference is present (the build container), tests/golden/gru_*.npz must be exactly what
tests/golden/make_gru_golden.py produces from it: the fixtures ARE outputs of the reference's own `SepConvGRU` and `ConvGRU`, not
hand-edited arrays.  Skipped where the reference does not exist; the generator runs in a subprocess."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/ggrt"), reason="the reference tree is not on this machine")


def test_gru_fixtures_are_what_the_generator_produces(tmp_path):
    env = dict(os.environ, GGR_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS="4")
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_gru_golden.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "gru_*.npz")))
    assert len(names) == 4 and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(tmp_path), "gru_*.npz")))
    for n in names:
        a, b = np.load(os.path.join(GOLDEN, n), allow_pickle=False), np.load(os.path.join(str(tmp_path), n), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), n
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (n, k)
            if k.startswith("g_") or k == "out":        # float64 results (a thread count may change a summation order)
                np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-13, err_msg=f"{n}:{k}")
            else:                                        # inputs and parameters: to the bit
                assert np.array_equal(a[k], b[k]), (n, k)
