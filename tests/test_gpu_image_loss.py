"""`fused_image_loss` / `fused_ssim` (csrc/image_loss.hip) on the GPU against the restatement of GGRt's `img2mse` and `ssim`
(tests/image_loss_reference.py, pinned to the reference's own modules by tests/test_image_loss_reference.py).

Three routes per case: `ref` the restatement in float64 on the CPU, `t32` the restatement in float32 on the device, `ker` the
kernel.  The bar for mse, ssim and both gradients is e_kernel <= max(4 * e_torch32, 1e-6) with e = |x - ref| / |ref| for mse,
|x - ref| for ssim (its scale is 1) and max|x - ref| / max|ref| for a gradient; every figure is printed before it is asserted.

The kernel's tile is T_h x T_w = 16 x 32 pixels of one (b, c) plane (halo 5 at window 11), so the shapes are: H and W below, at and
just above the halo and the window — (1,1), (5,6), (10,11), (11,12), (7,5); H at 15, 16, 17, 33 and W at 31, 32, 33, 65, each
direction on its own, and both at once; C in {1, 3, 4}, B in {1, 2, 3}, windows 1, 3, 7, 11, with and without a mask, size_average
on and off; and GGRt's own [2, 3, 352, 480].  The inputs are make_image_case's (pred = target + noise, SSIM 0.71 to 0.998).
Every buffer the launches must write whole is filled with NaN before the launch (`splatting._IMAGE_LOSS_POISON`)."""
import functools

import pytest
import torch

from tests.image_loss_reference import NOISES, image_loss_reference, make_image_case, run_image_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"

SMALL = [(1, 1), (5, 6), (10, 11), (11, 12), (7, 5)]
TILE_H = [(15, 9), (16, 9), (17, 9), (33, 9)]
TILE_W = [(6, 31), (6, 32), (6, 33), (6, 65)]
BOTH = [(17, 33), (33, 65)]


def _cases():
    out = []
    for i, (h, w) in enumerate(SMALL + TILE_H + TILE_W + BOTH):     # window 11: every shape
        out.append((1 + (i // 2) % 3, (1, 3, 4)[i % 3], h, w, 11, (h, w) != (1, 1) and i % 2 == 1, i % 4 < 2, NOISES[i % 3]))
    for j, ws in enumerate((1, 3, 7)):                              # the other windows: below, across and beyond the tile
        for i, (h, w) in enumerate([(7, 5), (17, 33), (33, 65)]):
            out.append((1 + (i + j) % 3, (4, 3, 1)[(i + j) % 3], h, w, ws, (i + j) % 2 == 0, i != 1, NOISES[(i + j) % 3]))
    out.append((2, 3, 352, 480, 11, True, True, 0.1))               # GGRt's own
    return out


CASES = _cases()
_id = lambda c: "b{}c{}_{}x{}_w{}_{}_{}_n{}".format(*c[:5], "masked" if c[5] else "plain", "mean" if c[6] else "per_image", c[7])


@pytest.fixture(autouse=True)
def _poisoned_buffers():
    from ggrt_official_amd import splatting
    splatting._IMAGE_LOSS_POISON = True
    yield
    splatting._IMAGE_LOSS_POISON = False


def kernel(pred, target, mask, window_size=11, size_average=True):
    from ggrt_official_amd import fused_image_loss
    return fused_image_loss(pred, target, mask, window_size=window_size, size_average=size_average)


@functools.lru_cache(maxsize=None)
def _routes(case, use=("mse", "ssim")):
    """(the case, ref, t32): computed once per case and shared; nothing modifies them"""
    b, c, h, w, ws, masked, size_average, noise = case
    data = make_image_case(b, c, h, w, noise, 1000 + 7 * h + w + ws, masked)
    ref = run_image_loss(image_loss_reference, data, torch.float64, "cpu", ws, size_average, use)
    t32 = run_image_loss(image_loss_reference, data, torch.float32, DEV, ws, size_average, use)
    return data, ref, t32


def _err(k, x, ref):
    x, ref = x.detach().double().cpu(), ref.double().cpu()
    if k == "mse":
        return float(((x - ref).abs() / ref.abs()).max())
    if k == "ssim":
        return float((x - ref).abs().max())
    return float((x - ref).abs().max() / ref.abs().max())


def _bar(got, ref, t32, keys, what):
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, (what, k)
        assert float(ref[k].abs().max()) > 0, (what, k)
        e_k, e_t = _err(k, got[k], ref[k]), _err(k, t32[k], ref[k])
        print(f"{what} {k}: e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
    for k in keys:
        e_k, e_t = _err(k, got[k], ref[k]), _err(k, t32[k], ref[k])
        assert e_k <= max(4 * e_t, 1e-6), (what, k, e_k, e_t)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_against_float64_within_the_float32_bar(case):
    data, ref, t32 = _routes(case)
    got = run_image_loss(kernel, data, torch.float32, DEV, case[4], case[6])
    _bar(got, ref, t32, ("mse", "ssim", "d_pred", "d_target"), _id(case))


@pytest.mark.parametrize("use", [("mse",), ("ssim",), ("mse", "ssim")], ids=lambda u: "+".join(u))
def test_a_field_without_an_upstream_gradient_contributes_nothing(use):
    case = (2, 3, 17, 33, 11, True, False, 0.1)
    data, ref, t32 = _routes(case, use)
    got = run_image_loss(kernel, data, torch.float32, DEV, 11, False, use)
    _bar(got, ref, t32, ("d_pred", "d_target"), "only " + "+".join(use))
    # SSIM is symmetric and the MSE term antisymmetric; with mse alone the target's gradient is the negated pred's, to the bit
    if use == ("mse",):
        assert torch.equal(got["d_target"], -got["d_pred"])


def test_pred_alone_gets_its_gradient_when_the_target_needs_none():
    case = (2, 3, 17, 33, 11, True, False, 0.1)
    data, _, _ = _routes(case)
    both = run_image_loss(kernel, data, torch.float32, DEV, 11, False)
    one = run_image_loss(kernel, data, torch.float32, DEV, 11, False, target_grad=False)
    assert "d_target" not in one and torch.equal(one["d_pred"], both["d_pred"]) and torch.equal(one["mse"], both["mse"])


def test_chw_input_is_the_b1_call_and_a_repeat_is_bit_equal():
    data = make_image_case(1, 3, 33, 65, 0.1, 1100, True)
    a = run_image_loss(kernel, data, torch.float32, DEV)
    again = run_image_loss(kernel, data, torch.float32, DEV)
    flat = dict(data, pred=data["pred"][0], target=data["target"][0], mask=data["mask"][0])
    chw = run_image_loss(kernel, flat, torch.float32, DEV)
    for k in a:
        assert torch.isfinite(a[k]).all() and float(a[k].abs().max()) > 0
        assert torch.equal(a[k], again[k]), k
        assert torch.equal(a[k].reshape(chw[k].shape), chw[k]), k
    assert a["mse"].shape == () and chw["d_pred"].shape == (3, 33, 65)
    # the big case too: partial sums of 1980 workgroups in a fixed order
    data, _, _ = _routes(CASES[-1])
    x, y = (run_image_loss(kernel, data, torch.float32, DEV) for _ in range(2))
    for k in x:
        assert torch.equal(x[k], y[k]), k


def test_fused_ssim_has_the_reference_signature_and_takes_strided_images():
    from ggrt_official_amd import fused_image_loss, fused_ssim
    data = make_image_case(2, 3, 20, 40, 0.1, 1110, False)
    pred, target = data["pred"].float().to(DEV), data["target"].float().to(DEV)
    want = fused_image_loss(pred, target, size_average=False)
    assert torch.equal(fused_ssim(pred, target, 11, False), want.ssim) and torch.equal(fused_ssim(pred, target), fused_image_loss(pred, target).ssim)
    hwc = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # a channels-last view of the same numbers
    assert not hwc.is_contiguous()
    got = fused_image_loss(hwc, target[:, :, :, :], size_average=False)
    assert torch.equal(got.mse, want.mse) and torch.equal(got.ssim, want.ssim)
    assert torch.equal(want.psnr, -10.0 * torch.log10(want.mse + 1e-6))
    ref = image_loss_reference(data["pred"], data["target"], None, 11, False)
    assert float((want.ssim.double().cpu() - ref[1]).abs().max()) <= 1e-5


def test_an_all_zero_mask_gives_exact_zeros():
    data = make_image_case(2, 3, 17, 33, 0.3, 1120, True)
    data["mask"] = torch.zeros_like(data["mask"])
    for size_average in (True, False):
        got = run_image_loss(kernel, data, torch.float32, DEV, 11, size_average, ("mse",))
        assert torch.equal(got["mse"], torch.zeros_like(got["mse"]))
        assert torch.equal(got["d_pred"], torch.zeros_like(got["d_pred"])) and torch.equal(got["d_target"], torch.zeros_like(got["d_target"]))


def test_equal_images_give_zero_mse_and_unit_ssim():
    data = make_image_case(2, 3, 33, 65, 0.1, 1130, True)
    data["pred"] = data["target"].clone()
    got = run_image_loss(kernel, data, torch.float32, DEV, 11, False)
    assert torch.equal(got["mse"], torch.zeros_like(got["mse"]))
    assert float((got["ssim"].double() - 1).abs().max()) <= 1e-6
    # (the exact SSIM gradient is 0 there and float32 returns rounding noise: only finiteness is asked)
    assert torch.isfinite(got["d_pred"]).all() and torch.isfinite(got["d_target"]).all()


def test_a_nan_pixel_gives_non_finite_losses_and_the_call_returns():
    data = make_image_case(1, 3, 33, 65, 0.1, 1140, False)
    data["pred"][0, 1, 16, 32] = float("nan")
    got = run_image_loss(kernel, data, torch.float32, DEV)
    torch.cuda.synchronize()
    assert not torch.isfinite(got["mse"]).any() and not torch.isfinite(got["ssim"]).any()
    bad = ~torch.isfinite(got["d_pred"][0])
    assert bool(bad[1, 16, 32]) and not bool(bad[0].any()) and not bool(bad[2].any())      # the NaN stays in its own plane
    data["pred"][0, 1, 16, 32] = float("inf")
    got = run_image_loss(kernel, data, torch.float32, DEV)
    torch.cuda.synchronize()
    assert not torch.isfinite(got["mse"]).any() and not torch.isfinite(got["ssim"]).any()


def test_every_refusal_names_its_argument():
    from ggrt_official_amd import fused_image_loss
    x = torch.rand(2, 3, 8, 9, device=DEV)
    m = torch.ones(2, 8, 9, device=DEV)
    with pytest.raises(ValueError, match="pred.*float32"):
        fused_image_loss(x.double(), x)
    with pytest.raises(ValueError, match="target.*float32"):
        fused_image_loss(x, x.half())
    with pytest.raises(ValueError, match="mask.*float32"):
        fused_image_loss(x, x, m.bool())
    with pytest.raises(RuntimeError, match="target.*GPU only"):
        fused_image_loss(x, x.cpu())
    with pytest.raises(RuntimeError, match="mask.*GPU only"):
        fused_image_loss(x, x, m.cpu())
    with pytest.raises(ValueError, match="target.*shape of pred"):
        fused_image_loss(x, x[:, :, :, :8])
    with pytest.raises(ValueError, match="mask"):
        fused_image_loss(x, x, m[:, None].expand(2, 3, 8, 9))
    with pytest.raises(ValueError, match="mask"):
        fused_image_loss(x, x, m[0])
    with pytest.raises(ValueError, match="mask"):
        fused_image_loss(x[0], x[0], m)
    for ws in (0, 2, 10, 13, -1):
        with pytest.raises(ValueError, match="window_size"):
            fused_image_loss(x, x, window_size=ws)
    for shape in ((0, 3, 8, 9), (2, 0, 8, 9), (2, 3, 0, 9), (2, 3, 8, 0)):
        with pytest.raises(ValueError, match="pred.*no elements"):
            fused_image_loss(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError, match="pred"):
        fused_image_loss(x[0, 0], x[0, 0])
    with pytest.raises(RuntimeError, match="mask requires grad"):
        fused_image_loss(x, x, m.clone().requires_grad_(True))
