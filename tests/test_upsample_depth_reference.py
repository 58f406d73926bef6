"""The torch restatement of the convex depth upsampling (tests/upsample_depth_reference.py) against fixtures made by the reference's
own `DepthPoseNet.upsample_depth` and `disp_to_depth` (tests/golden/make_upsample_depth_golden.py): in float64 it equals them to
1e-12, the value (with and without the affine map) and both gradients; it passes gradcheck; its resize is `F.interpolate`'s; and at
the identity size it returns `up` to the bit.  Also the cases the GPU tests run."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.upsample_depth_reference import (INPUTS, bilinear_resize, convex_upsample, make_upsample_case, run_upsample_depth,
                                            upsample_depth_reference)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f)[len("upsample_depth_"):-4] for f in glob.glob(os.path.join(GOLDEN, "upsample_depth_*.npz")))

# name: (N, h, w, r, (Ho, Wo) or None for the identity size, seed) — the GPU tests' shapes: the three fixture shapes, an identity
# size over more than one 64-cell tile's worth of sub-pixels, r = 1 (one sub-pixel: three of the four waves idle), one output pixel,
# and a 70-cell row that crosses a wave
GPU_CASES = {
    "n2_r8_down_rows": (2, 3, 5, 8, (21, 40), 910),
    "n1_r4_up": (1, 2, 3, 4, (13, 29), 911),
    "n1_r2_one_cell": (1, 1, 1, 2, (2, 2), 912),
    "n3_r8_identity": (3, 5, 9, 8, None, 913),
    "n2_r1": (2, 4, 7, 1, (6, 5), 914),
    "one_output_pixel": (2, 3, 4, 4, (1, 1), 915),
    "row_crosses_a_wave": (1, 3, 70, 2, (7, 131), 916),
}
FULL_CASE = (4, 48, 63, 8, (378, 504), 917)
DISP_RANGE = (0.1, 100.0)


def _load(name):
    z = np.load(os.path.join(GOLDEN, f"upsample_depth_{name}.npz"), allow_pickle=False)
    case = {k: torch.from_numpy(z[k]) for k in INPUTS + ("g",)}
    return z, case, int(z["ratio"]), tuple(int(x) for x in z["image_size"])


def test_there_are_three_fixtures_of_the_shapes_the_issue_names():
    assert FIXTURES == ["n1_r2_one_cell", "n1_r4_up", "n2_r8_down_rows"]
    shapes = {n: (tuple(_load(n)[1]["mask"].shape), _load(n)[3]) for n in FIXTURES}
    assert shapes == {"n2_r8_down_rows": ((2, 576, 3, 5), (21, 40)), "n1_r4_up": ((1, 144, 2, 3), (13, 29)), "n1_r2_one_cell": ((1, 36, 1, 1), (2, 2))}
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f"upsample_depth_{n}.npz")) < 400 * 1024
        assert tuple(_load(n)[0]["disp_range"]) == DISP_RANGE


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_equals_the_reference(name):
    z, case, r, size = _load(name)
    got = run_upsample_depth("torch", case, torch.float64, "cpu", ratio=r, image_size=size)
    np.testing.assert_allclose(got["out"].numpy(), z["out64"], rtol=0, atol=1e-12)
    for k in INPUTS:
        np.testing.assert_allclose(got["g_" + k].numpy(), z[f"g_{k}64"], rtol=0, atol=1e-12, err_msg=k)
    disp = run_upsample_depth("torch", case, torch.float64, "cpu", need=(), ratio=r, image_size=size, disp_range=DISP_RANGE)
    np.testing.assert_allclose(disp["out"].numpy(), z["disp64"], rtol=0, atol=1e-12)
    # the affine map's gradients are those of the plain map times its slope
    lo, hi = 1.0 / DISP_RANGE[1], 1.0 / DISP_RANGE[0]
    both = run_upsample_depth("torch", case, torch.float64, "cpu", ratio=r, image_size=size, disp_range=DISP_RANGE)
    for k in INPUTS:
        np.testing.assert_allclose(both["g_" + k].numpy(), (hi - lo) * z[f"g_{k}64"], rtol=0, atol=1e-11, err_msg=k)


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_restatement_is_close_to_the_reference_in_float32(name):
    z, case, r, size = _load(name)
    got = run_upsample_depth("torch", case, torch.float32, "cpu", ratio=r, image_size=size)
    np.testing.assert_allclose(got["out"].numpy(), z["out32"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got["g_depth"].numpy(), z["g_depth32"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("opts", [dict(ratio=2, image_size=(5, 9)), dict(ratio=2, image_size=None, disp_range=(0.1, 100.0)), dict(ratio=1, image_size=(1, 1))])
def test_gradcheck(opts):
    case = make_upsample_case(2, 2, 3, opts["ratio"], opts["image_size"], 920)
    d, m = case["depth"].clone().requires_grad_(True), case["mask"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d, m: upsample_depth_reference(d, m, **opts), (d, m), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("sizes", [((24, 40), (21, 40)), ((8, 12), (13, 29)), ((2, 2), (2, 2)), ((3, 5), (1, 1)), ((1, 1), (4, 3)), ((384, 504), (378, 504))])
def test_the_resize_is_torchs(sizes, dtype):
    (H, W), size = sizes
    up = torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(921), dtype=dtype)
    want = F.interpolate(up, size=size, mode="bilinear", align_corners=True)
    assert float((bilinear_resize(up, size) - want).abs().max()) <= (1e-15 if dtype == torch.float64 else 2e-7)


def test_at_the_identity_size_the_result_is_up_to_the_bit():
    case = make_upsample_case(2, 3, 4, 4, None, 922)
    for dtype in (torch.float32, torch.float64):
        d, m = case["depth"].to(dtype), case["mask"].to(dtype)
        up = convex_upsample(d, m, 4)
        assert torch.equal(upsample_depth_reference(d, m, ratio=4), up) and torch.equal(upsample_depth_reference(d, m, ratio=4, image_size=(12, 16)), up)
        assert torch.equal(F.interpolate(up, size=(12, 16), mode="bilinear", align_corners=True), up)


def test_an_all_zero_mask_is_the_zero_padded_box_mean():
    d = torch.ones(1, 1, 4, 5, dtype=torch.float64)
    out = upsample_depth_reference(d, torch.zeros(1, 36, 4, 5, dtype=torch.float64), ratio=2)
    want = F.avg_pool2d(d, 3, 1, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert float((out - want).abs().max()) <= 1e-15
    assert abs(float(out[0, 0, 0, 0]) - 4 / 9) < 1e-15 and abs(float(out[0, 0, 0, 3]) - 6 / 9) < 1e-15 and abs(float(out[0, 0, 3, 3]) - 1) < 1e-15


def test_gpu_cases_cover_the_shapes_the_issue_names():
    shapes = {(N, h, w, r, size) for N, h, w, r, size, _ in GPU_CASES.values()}
    assert {(2, 3, 5, 8, (21, 40)), (1, 2, 3, 4, (13, 29)), (1, 1, 1, 2, (2, 2)), (3, 5, 9, 8, None), (1, 3, 70, 2, (7, 131))} <= shapes
    assert any(r == 1 and (N, h, w) == (2, 4, 7) for N, h, w, r, _ in shapes) and any(size == (1, 1) for *_, size in shapes)
    assert FULL_CASE[:5] == (4, 48, 63, 8, (378, 504))
