"""The torch restatement of the convex depth upsampling (tests/upsample_depth_reference.py) against fixtures made by the reference's
own `DepthPoseNet.upsample_depth` and `disp_to_depth` (tests/golden/make_upsample_depth_golden.py): in float64 it equals them to
1e-12, the value (with and without the affine map) and both gradients; it passes gradcheck; its resize is `F.interpolate`'s; and at
the identity size it returns `up` to the bit.  Also the cases the GPU tests run: `GPU_CASES`, and `RESIZE_CASES` with the checks
that each of those is the regime its name claims."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.upsample_depth_reference import (INPUTS, _axis, bilinear_resize, convex_upsample, make_upsample_case, run_upsample_depth,
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

# the resize regimes of the backward gather's destination window (`reach()` in csrc/upsample_depth.hip) and the tile seams, same
# tuple form: a strong downscale (most `up` pixels reached by no destination; 66 cells = 2 tiles, N = 2), a strong upscale (windows
# over most of the output), one destination index on one axis only, one source index on an axis, scales at which every source
# coordinate is an integer (31 and 3: every l1 is 0), an output one pixel larger and smaller than `up`, and N > 1 with several
# tiles whose seams fall mid-row (133 cells at r = 8, identity and resized; 135 cells at r = 3, r r = 9 over 4 waves)
RESIZE_CASES = {
    "strong_down": (2, 6, 11, 8, (3, 5), 960),
    "strong_up": (2, 1, 2, 2, (33, 47), 961),
    "one_row_out": (1, 3, 4, 4, (1, 29), 962),
    "one_col_out": (1, 3, 4, 4, (23, 1), 963),
    "one_row_in": (2, 1, 5, 1, (7, 9), 964),
    "one_col_in": (2, 5, 1, 1, (4, 6), 965),
    "integer_sources": (1, 4, 8, 8, (2, 22), 966),
    "one_larger": (1, 3, 9, 8, (25, 73), 967),
    "one_smaller": (1, 3, 9, 8, (23, 71), 968),
    "seams_r8_identity": (3, 7, 19, 8, None, 969),
    "seams_r8_resized": (3, 7, 19, 8, (50, 161), 970),
    "seams_r3": (2, 5, 27, 3, (11, 90), 971),
}
RESIZE_PAIRS = [((r * h, r * w), size if size is not None else (r * h, r * w)) for _, h, w, r, size, _ in RESIZE_CASES.values()]


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
@pytest.mark.parametrize("sizes", [((24, 40), (21, 40)), ((8, 12), (13, 29)), ((2, 2), (2, 2)), ((3, 5), (1, 1)), ((1, 1), (4, 3)), ((384, 504), (378, 504))]
                         + RESIZE_PAIRS)
def test_the_resize_is_torchs(sizes, dtype):
    (H, W), size = sizes
    up = torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(921), dtype=dtype)
    want = F.interpolate(up, size=size, mode="bilinear", align_corners=True)
    assert float((bilinear_resize(up, size) - want).abs().max()) <= (1e-15 if dtype == torch.float64 else 2e-7)


@pytest.mark.parametrize("name", ["one_row_in", "strong_up"])
def test_gradcheck_at_the_resize_regimes(name):
    N, h, w, r, size, seed = RESIZE_CASES[name]
    case = make_upsample_case(N, h, w, r, size, seed)
    d, m = case["depth"].clone().requires_grad_(True), case["mask"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d, m: upsample_depth_reference(d, m, ratio=r, image_size=size), (d, m), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_integer_sources_has_no_second_tap_in_float32():
    """The case is the regime it names: scales 31 and 3 exactly, every float32 source coordinate an integer, so the second tap has
    weight 0 at every destination and the last source index is the FIRST tap of the last destination."""
    _, h, w, r, (Ho, Wo), _ = RESIZE_CASES["integer_sources"]
    for n_in, n_out, scale in ((r * h, Ho, 31), (r * w, Wo, 3)):
        i0, i1, l0, l1 = _axis(n_in, n_out, torch.float32, "cpu")
        assert torch.equal(l1, torch.zeros(n_out)) and torch.equal(l0, torch.ones(n_out))
        assert i0.tolist() == [scale * o for o in range(n_out)] and int(i0[-1]) == n_in - 1 == int(i1[-1])


def test_strong_down_leaves_most_of_the_mask_gradient_exactly_zero():
    """The condition the GPU test of this case rests on, from the restatement alone in float32: more than half of dL/dmask is an
    exact zero (an `up` pixel no destination reaches), and whole (cell, sub-pixel) groups of nine taps are zero or nonzero together."""
    N, h, w, r, size, seed = RESIZE_CASES["strong_down"]
    got = run_upsample_depth("torch", make_upsample_case(N, h, w, r, size, seed), torch.float32, "cpu", ratio=r, image_size=size, disp_range=DISP_RANGE)
    zero = got["g_mask"].reshape(N, 9, r * r, h, w) == 0
    share = float(zero.double().mean())
    print(f"strong_down: {share:.4f} of dL/dmask is exactly zero")
    assert 0.5 < share < 1.0
    assert torch.equal(zero.all(1), zero.any(1))
    # rows 0, 23, 24, 47 and columns 0, 21, 22, 43, 44, 65, 66, 87 of the 48 x 88 `up` carry a weight: 32 of 4224 pixels
    assert int((~zero.all(1)).sum()) == N * 32


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
    assert {k: v[:5] for k, v in RESIZE_CASES.items()} == {
        "strong_down": (2, 6, 11, 8, (3, 5)), "strong_up": (2, 1, 2, 2, (33, 47)), "one_row_out": (1, 3, 4, 4, (1, 29)),
        "one_col_out": (1, 3, 4, 4, (23, 1)), "one_row_in": (2, 1, 5, 1, (7, 9)), "one_col_in": (2, 5, 1, 1, (4, 6)),
        "integer_sources": (1, 4, 8, 8, (2, 22)), "one_larger": (1, 3, 9, 8, (25, 73)), "one_smaller": (1, 3, 9, 8, (23, 71)),
        "seams_r8_identity": (3, 7, 19, 8, None), "seams_r8_resized": (3, 7, 19, 8, (50, 161)), "seams_r3": (2, 5, 27, 3, (11, 90))}
    seeds = [c[5] for c in list(GPU_CASES.values()) + list(RESIZE_CASES.values())] + [FULL_CASE[5]]
    assert len(set(seeds)) == len(seeds)
    assert RESIZE_PAIRS[:2] == [((48, 88), (3, 5)), ((2, 4), (33, 47))] and ((56, 152), (56, 152)) in RESIZE_PAIRS and len(RESIZE_PAIRS) == len(RESIZE_CASES)
    # what the names claim: tiles of 64 flattened cells
    tiles = lambda name: -(-RESIZE_CASES[name][1] * RESIZE_CASES[name][2] // 64)
    assert (tiles("strong_down"), tiles("seams_r8_identity"), tiles("seams_r8_resized"), tiles("seams_r3")) == (2, 3, 3, 3)
    assert all(RESIZE_CASES[n][2] % 64 and 64 % RESIZE_CASES[n][2] for n in ("seams_r8_identity", "seams_r8_resized", "seams_r3"))       # seams mid-row
