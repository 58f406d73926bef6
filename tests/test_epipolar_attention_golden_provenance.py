"""tests/golden/epi_attention_*.npz (made by tests/golden/make_epipolar_attention_golden.py from the reference's own
`Attention`): the files hold the documented keys with consistent shapes and dtypes, both precisions, the cases the generator
lists, and inputs that `make_case` of tests/epipolar_attention_reference.py reproduces from the recorded seed."""
import numpy as np
import pytest
import torch

from tests.epipolar_attention_reference import make_case
from tests.test_epipolar_attention_reference import LEAVES, NAMES, load_golden

# name: (N, S, dim, kv_dim, H, D, project_out) — as in the generator
SHAPES = {"two_heads": (5, 4, 6, 6, 2, 3, True), "four_heads": (3, 8, 8, 5, 4, 2, True), "no_projection": (4, 5, 6, 4, 1, 6, False)}


@pytest.mark.parametrize("name", NAMES)
def test_keys_shapes_dtypes_and_seeded_inputs(name):
    case, z = load_golden(name)
    n, s, dim, kv_dim, heads, d, project_out = SHAPES[name]
    inner = heads * d
    shapes = {"x": (n, 1, dim), "z": (n, s, kv_dim), "w_q": (inner, dim), "w_kv": (2 * inner, kv_dim)}
    if project_out:
        shapes.update(w_out=(dim, inner), b_out=(dim,))
    else:
        assert heads == 1 and d == dim and case["w_out"] is None and case["b_out"] is None
    assert case["heads"] == heads
    want = set(shapes) | {"g_out", "heads", "seed"} | {p + t for p in ["out"] + ["g_" + k for k in shapes] for t in ("32", "64")}
    assert set(z.files) == want
    assert z["g_out"].shape == (n, 1, dim) and z["g_out"].dtype == np.float64
    for k, shape in shapes.items():
        assert z[k].shape == shape and z[k].dtype == np.float64, k
        for tag, dtype in (("32", np.float32), ("64", np.float64)):
            g = z["g_" + k + tag]
            assert g.shape == shape and g.dtype == dtype and np.isfinite(g).all(), (k, tag)
    for tag, dtype in (("32", np.float32), ("64", np.float64)):
        assert z["out" + tag].shape == (n, 1, dim) and z["out" + tag].dtype == dtype
    again = make_case(n, s, dim, kv_dim, heads, d, case["seed"], project_out)
    for k in LEAVES + ("g_out",):
        assert (again[k] is None) == (case[k] is None)
        if again[k] is not None:
            assert torch.equal(again[k], case[k]), k
    for f in z.files:
        assert z[f].dtype in (np.float32, np.float64, np.int64)      # (only arrays of numbers travel)
