"""tests/image_loss_reference.py against the reference's own `ssim` and `img2mse` (tests/golden/image_loss_*.npz, written by
tests/golden/make_image_loss_golden.py from the reference's modules): the restatement in float64 reproduces the float64 fixtures to
1e-12 — results and the gradients with respect to both images — its autograd passes `gradcheck`, and the separable application of
the window, which is what the kernel does, equals the 2-D window to 1e-12 in float64.  No GPU."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.image_loss_reference import NOISES, gaussian, image_loss_reference, make_image_case, mse2psnr, run_image_loss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(f)[len("image_loss_"):-len(".npz")] for f in glob.glob(os.path.join(GOLDEN, "image_loss_*.npz")))


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, f"image_loss_{name}.npz"), allow_pickle=False)
    t = lambda k: torch.from_numpy(z[k]).double() if k in z.files else None
    case = dict(pred=t("pred"), target=t("target"), mask=t("mask"), g_mse=t("g_mse"), g_ssim=t("g_ssim"))
    return z, case, int(z["window_size"]), bool(z["size_average"])


def test_the_fixtures_are_the_four_cases():
    assert NAMES == ["b1c1_tiny", "b1c4_window7", "b2c3_masked", "b3c3_per_image"]
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"image_loss_{name}.npz")) < 64 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_in_float64(name):
    z, case, window_size, size_average = load_fixture(name)
    got = run_image_loss(image_loss_reference, case, torch.float64, "cpu", window_size, size_average)
    assert got["mse"].shape == (() if size_average else (case["pred"].shape[0],))
    for k in ("mse", "ssim", "d_pred", "d_target"):
        ref = z[k + "64"]
        assert ref.dtype == np.float64 and np.abs(ref).max() > 0
        np.testing.assert_allclose(got[k].numpy(), ref, rtol=0, atol=1e-12, err_msg=f"{name}:{k}")
    # the reference's own float32 run: the scale of the float32 error the GPU test's bar is built on
    for k in ("d_pred", "d_target"):
        e = np.abs(z[k + "32"].astype(np.float64) - z[k + "64"]).max() / np.abs(z[k + "64"]).max()
        assert e < 1e-4, (name, k, e)
    assert np.array_equal(gaussian(window_size).numpy(), z["window"])


@pytest.mark.parametrize("name", NAMES)
def test_separable_window_equals_the_2d_window_in_float64(name):
    z, case, window_size, size_average = load_fixture(name)
    # (the reference's 2-D window holds the float32 products of the taps; the separable route cannot equal THOSE entries below
    #  2^-24 relative, so the comparison is with the same taps' outer product in float64: the same window, another order of summation)
    a = run_image_loss(image_loss_reference, case, torch.float64, "cpu", window_size, size_average, separable="outer")
    b = run_image_loss(image_loss_reference, case, torch.float64, "cpu", window_size, size_average, separable=True)
    for k in ("mse", "ssim", "d_pred", "d_target"):
        assert float(a[k].abs().max()) > 0
        assert float((a[k] - b[k]).abs().max()) <= 1e-12, (name, k)


def test_gradcheck_on_a_tiny_case():
    case = make_image_case(2, 2, 6, 5, 0.1, 910, True)
    for size_average in (True, False):
        fn = lambda p, t: torch.stack([r.sum() for r in image_loss_reference(p, t, case["mask"], 5, size_average)])
        assert torch.autograd.gradcheck(fn, (case["pred"].clone().requires_grad_(True), case["target"].clone().requires_grad_(True)),
                                        eps=1e-6, atol=1e-7, rtol=1e-5)


def test_the_inputs_sit_where_the_issue_measured_them():
    """SSIM of make_image_case's images: 0.998, 0.95-0.97 and 0.71 at the three noise levels (not the 0.1 of independent images)."""
    want = {0.02: (0.99, 1.0), 0.1: (0.93, 0.98), 0.3: (0.6, 0.8)}
    for noise in NOISES:
        case = make_image_case(1, 3, 40, 48, noise, 920, False)
        _, s = image_loss_reference(case["pred"], case["target"])
        assert want[noise][0] < float(s) < want[noise][1], (noise, float(s))


def test_mask_semantics_and_psnr():
    case = make_image_case(2, 3, 9, 8, 0.1, 930, True)
    zero = torch.zeros_like(case["mask"])
    mse, _ = image_loss_reference(case["pred"], case["target"], zero)
    assert float(mse) == 0.0
    ones = torch.ones_like(case["mask"])
    a, _ = image_loss_reference(case["pred"], case["target"], ones)
    b, _ = image_loss_reference(case["pred"], case["target"], None)
    assert abs(float(a) - float(b)) <= 1e-8 * float(b)       # (the 1e-6 in the masked denominator)
    assert abs(float(mse2psnr(b)) + 10 * np.log10(float(b) + 1e-6)) < 1e-12
