"""The fused epipolar sampler (csrc/epipolar.hip, `fused_epipolar_sampler`) against its float64 restatement
(tests/epipolar_reference.py), forward and backward.

Three routes: the restatement in float64 on the CPU (`ref`), the restatement in float32 on the device (`t32`), the kernels
(`ker`).  `valid` must be equal on EVERY ray in all three (the cases obey the margin rule of `make_case`).  For every float output
and for dL/dimages  e = max|x − ref64| / max|ref64|  and the bar is  e_kernel <= max(4·e_torch32, 1e-6).  Features of invalid
rays are exact zeros.  The loss is Σ features · fixed random weights.

Shapes: the smallest at which the kernels can go wrong.  A wave (64 lanes) owns one (view, other view, ray) and walks its samples
with the lanes across the channels, so c = 1, 3, 64, 127, 128, 130 sit below, at and above one and two trips of the channel loop
(and below / at / above the layout kernels' 32-channel tile); one lane owns one sample for the coordinates and the depth, so
s = 1, 2, 31, 32, 33, 64 walk that lane mask up to the full wave and the sample loop's unrolling by 4.  A workgroup is four
waves = four pair-rays: the grids 1×1 (2 pair-rays at v = 2: half a workgroup), 1×7, 5×7, 11×13, 16×16 and 65×3 put the number of
pair-rays below, at (16×16·2 = 128 workgroups exactly) and off a multiple of four, and h·w = 1, 7, 35, 143, 195, 256 below, off
and at a multiple of the layout kernels' 32-pixel tile.  v = 3, 4 put the sampled view o on both sides of the casting view and
give the other-view axis a stride; b = 2 gives the batch one."""
import pytest
import torch
import torch.nn.functional as F

from tests.epipolar_reference import FLOAT_OUTPUTS, epipolar_reference, make_case, other_views, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _as_dict(out):
    return out if isinstance(out, dict) else {k: getattr(out, k) for k in FLOAT_OUTPUTS + ("valid",)}


def _weights(case, seed):
    b, v, c, h, w = case["images"].shape
    win = case["ray_window"]
    r = h * w if win is None else (win[1] - win[0]) * (win[3] - win[2])
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.randn((b, v, v - 1, r, case["num_samples"], c), generator=gen, dtype=torch.float64)


def _run(fn, case, dtype, device, weights, twice=False):
    """every output and dL/dimages of one route, as float64 CPU tensors"""
    images = case["images"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    out = _as_dict(run_case(fn, dict(case, images=images), dtype, device))
    loss = (out["features"] * weights.to(device=device, dtype=dtype)).sum()
    (g,) = torch.autograd.grad(loss, [images], retain_graph=twice, allow_unused=True)
    res = {k: out[k].detach().double().cpu() for k in FLOAT_OUTPUTS}
    res["valid"] = out["valid"].detach().cpu()
    res["d_images"] = torch.zeros_like(case["images"]) if g is None else g.double().cpu()
    if twice:
        res["d_images_again"] = torch.autograd.grad(loss, [images])[0].double().cpu()
    return res


def _three_routes(case, seed):
    from ggrt_official_amd import fused_epipolar_sampler
    w = _weights(case, seed)
    return (_run(epipolar_reference, case, torch.float64, "cpu", w), _run(epipolar_reference, case, torch.float32, DEV, w),
            _run(fused_epipolar_sampler, case, torch.float32, DEV, w))


def _routes(b, v, h, w, c, s, family="default", window=None):
    key = (b, v, h, w, c, s, family, window)
    if key not in _CACHE:
        seed = 3 * b + 5 * v + 7 * h + 11 * w + 13 * c + 17 * s
        case = make_case(b, v, h, w, c, s, seed, family, window)
        _CACHE[key] = (case,) + _three_routes(case, seed)
    return _CACHE[key]


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def _hold_to_the_bar(ref, t32, ker, what="", all_invalid=False):
    assert ker["valid"].dtype == torch.bool and ker["valid"].shape == ref["valid"].shape
    assert torch.equal(ker["valid"], ref["valid"]), (what, int((ker["valid"] != ref["valid"]).sum()))
    assert torch.equal(t32["valid"], ref["valid"]), what
    dead = ~ref["valid"]
    assert float(ker["features"][dead].abs().sum()) == 0, what            # exact zeros on invalid rays
    for k in ("xy_sample", "xy_sample_near", "xy_sample_far"):
        assert float(ker[k][dead].abs().sum()) == 0, (what, k)
    bad = []
    for k in FLOAT_OUTPUTS + ("d_images",):
        r = ref[k]
        assert ker[k].shape == r.shape, (k, ker[k].shape, r.shape)
        if float(r.abs().max()) == 0:
            assert all_invalid and k in ("features", "xy_sample", "xy_sample_near", "xy_sample_far", "d_images"), k
            assert float(ker[k].abs().max()) == 0, k
            continue
        e_k, e_t = _err(ker[k], r), _err(t32[k], r)
        print(f"{what} {k:15s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad


CHANNELS = [(1, 3, 5, 7, c, 8) for c in (1, 3, 64, 127, 128, 130)]
SAMPLES = [(1, 2, 5, 7, 5, s) for s in (1, 2, 31, 32, 33, 64)]
VIEWS = [(1, 2, 11, 13, 4, 8), (1, 3, 11, 13, 4, 8), (1, 4, 5, 7, 4, 8), (2, 2, 5, 7, 4, 8), (2, 3, 5, 7, 4, 8)]
GRIDS = [(1, 2, h, w, 6, 8) for h, w in ((1, 1), (1, 7), (5, 7), (16, 16), (65, 3))]


@pytest.mark.parametrize("b,v,h,w,c,s", CHANNELS + SAMPLES + VIEWS + GRIDS)
def test_valid_outputs_and_gradient_match_the_float64_restatement(b, v, h, w, c, s):
    case, ref, t32, ker = _routes(b, v, h, w, c, s)
    assert ref["features"].shape == (b, v, v - 1, h * w, s, c) and ref["depth"].shape == (b, v, v - 1, h * w, s)
    _hold_to_the_bar(ref, t32, ker, f"b={b} v={v} {h}x{w} c={c} s={s} seed={case['seed']}")


@pytest.mark.parametrize("window", [(2, 7, 3, 9), (0, 4, 8, 13)])
def test_a_ray_window_casts_only_its_rays_and_keeps_the_maps_whole(window):
    """strictly inside the 11 × 13 frame, and touching its top and right edges"""
    case, ref, t32, ker = _routes(1, 3, 11, 13, 5, 8, "default", window)
    r = (window[1] - window[0]) * (window[3] - window[2])
    assert ker["features"].shape == (1, 3, 2, r, 8, 5) and ker["xy_ray"].shape == (1, 3, r, 2)
    _hold_to_the_bar(ref, t32, ker, f"window {window}")
    # the same rays of the whole grid give the same bits
    from ggrt_official_amd import fused_epipolar_sampler
    whole = _as_dict(run_case(fused_epipolar_sampler, dict(case, ray_window=None), torch.float32, DEV))
    rows = (torch.arange(window[0], window[1])[:, None] * 13 + torch.arange(window[2], window[3])[None]).reshape(-1)
    for k in ("features", "xy_sample", "depth"):
        assert torch.equal(whole[k][:, :, :, rows.to(DEV)].double().cpu(), ker[k]), k


def test_views_facing_away_from_each_other_give_zero_features_and_zero_gradient():
    case, ref, t32, ker = _routes(1, 2, 5, 7, 4, 8, "away")
    assert not bool(ref["valid"].any())
    _hold_to_the_bar(ref, t32, ker, "away", all_invalid=True)
    assert float(ker["features"].abs().max()) == 0 and float(ker["d_images"].abs().max()) == 0
    assert float(ref["depth"].abs().max()) > 0       # (the depth of an invalid ray is still the reference's: the lift of xy = 0)


@pytest.mark.parametrize("family", ["clipped", "inside"])
def test_segments_cut_by_the_frame_and_segments_wholly_inside(family):
    """`clipped`: most segments end at frame intersections; `inside`: most lie between the near and far projections"""
    case, ref, t32, ker = _routes(1, 2, 11, 13, 4, 8, family)
    det = run_case(epipolar_reference, case, details=True)
    both_points = (det["min_valid"] & det["max_valid"]).double().mean()
    assert (float(both_points) < 0.3) if family == "clipped" else (float(both_points) > 0.7), float(both_points)
    assert float(ref["valid"].double().mean()) > 0.5
    _hold_to_the_bar(ref, t32, ker, family)


def test_near_and_far_are_those_of_the_casting_view():
    """near = far / 2 per view, far differing by 4 from view to view: the sampled view's near / far would move every segment"""
    case, ref, t32, ker = _routes(1, 2, 5, 7, 4, 8, "nearfar")
    assert float((case["far"][0, 0] - case["far"][0, 1]).abs()) > 2 and torch.allclose(case["near"], case["far"] / 2)
    _hold_to_the_bar(ref, t32, ker, "nearfar")
    swapped = run_case(epipolar_reference, dict(case, near=case["near"].flip(1), far=case["far"].flip(1)))
    assert _err(swapped["xy_sample"], ref["xy_sample"]) > 1e-2


def test_two_backward_runs_agree_to_summation_order():
    case = make_case(1, 2, 11, 13, 16, 8, 77)
    from ggrt_official_amd import fused_epipolar_sampler
    ker = _run(fused_epipolar_sampler, case, torch.float32, DEV, _weights(case, 77), twice=True)
    assert float(ker["d_images"].abs().max()) > 0
    assert _err(ker["d_images_again"], ker["d_images"]) <= 1e-6


def test_features_equal_grid_sample_at_the_kernels_own_sample_points():
    """the bilinear convention pinned without the restatement: F.grid_sample(images[b, o], 2·xy_sample − 1) on the device"""
    from ggrt_official_amd import fused_epipolar_sampler
    case = make_case(1, 3, 11, 13, 7, 8, 78)
    out = _as_dict(run_case(fused_epipolar_sampler, case, torch.float32, DEV))
    images = case["images"].to(device=DEV, dtype=torch.float32)
    idx = other_views(3, DEV)
    maps = images[:, idx].reshape(6, 7, 11, 13)
    got = F.grid_sample(maps, (2 * out["xy_sample"] - 1).reshape(6, 143, 8, 2), mode="bilinear", padding_mode="zeros", align_corners=False)
    want = got.reshape(1, 3, 2, 7, 143, 8).permute(0, 1, 2, 4, 5, 3) * out["valid"][..., None, None]
    assert bool(out["valid"].any())
    # float32 rounding: a pixel coordinate below 16 has an ulp of 2^-20, and one ulp of difference in x or in y (a fused or an
    # unfused multiply-add on the way to it) moves a weight by as much and the result by at most 2·max|image| each; on top,
    # four products and three sums of the taps themselves, half an ulp of the largest each at most
    bound = (2 * 2 * 2.0 ** -20 + 4 * 2.0 ** -23) * float(images.abs().max())
    assert float((out["features"] - want).abs().max()) <= bound


def test_a_strided_view_of_the_feature_maps_is_read_in_place():
    from ggrt_official_amd import fused_epipolar_sampler
    case = make_case(1, 2, 5, 7, 6, 8, 79)
    dense = case["images"].to(device=DEV, dtype=torch.float32)
    wide = torch.randn(1, 2, 9, 5, 10, device=DEV)
    wide[:, :, 1:7, :, 2:9] = dense
    a = _as_dict(run_case(fused_epipolar_sampler, dict(case, images=dense), torch.float32, DEV))
    view = wide[:, :, 1:7, :, 2:9].requires_grad_(True)
    b_ = fused_epipolar_sampler(view, *(case[k].to(device=DEV, dtype=torch.float32) for k in ("extrinsics", "intrinsics", "near", "far")), 8)
    assert torch.equal(a["features"], b_.features)
    (g,) = torch.autograd.grad(b_.features.sum(), [view])
    assert g.shape == view.shape and float(g.abs().max()) > 0


def test_cameras_that_require_grad_are_refused():
    from ggrt_official_amd import fused_epipolar_sampler
    case = make_case(1, 2, 3, 4, 2, 4, 80)
    args = {k: case[k].to(device=DEV, dtype=torch.float32) for k in ("images", "extrinsics", "intrinsics", "near", "far")}
    for k in ("extrinsics", "intrinsics", "near", "far"):
        with pytest.raises(RuntimeError, match="camera gradients are not implemented"):
            fused_epipolar_sampler(**dict(args, **{k: args[k].clone().requires_grad_(True)}), num_samples=4)
    with pytest.raises(RuntimeError, match="num_samples"):
        fused_epipolar_sampler(**args, num_samples=65)
    with pytest.raises(ValueError):
        fused_epipolar_sampler(**args, num_samples=4, ray_window=(0, 4, 0, 4))
