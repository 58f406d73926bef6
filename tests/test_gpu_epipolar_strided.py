"""The fused epipolar sampler above its grid cap: the trips of `for (p = …; p < total; p += gridDim.x * WAVES)` in
`epipolar_fwd_kernel` and `epipolar_bwd_kernel` (csrc/epipolar.hip) beyond the first.

The grid is min(⌈pair-rays / 4⌉, kEpipolarMaxGroups = 4096) workgroups of WAVES = 4 waves and a wave owns one pair-ray per trip, so
a wave takes a second pair-ray only above 4096·4 = 16 384 pair-rays.  Two cases, the smallest that get there in the two ways that
matter:

  ragged  b = 235, v = 2, 5×7 rays: 235·2·1·35 = 16 450 pair-rays > 16 384.  66 of them are second trips: workgroups 0 … 15 whole
          and waves 0, 1 of workgroup 16 (16 450 is no multiple of 4); every other wave leaves the loop after one trip.
  even    b = 33, v = 2, 16×16 rays: 33·2·1·256 = 16 896 = 16 384 + 512: workgroups 0 … 127 take a second trip with all four waves.

A random camera case of 16 000 rays cannot obey the margin rule of `make_case` (some validity quantity always lands within 1e-4 of
its threshold), so each case repeats the cameras, near and far of an admissible b = 1 case over the batch and draws fresh images for
every element: the margin count is the small case's.  c = 3, s = 2 keep the outputs small; the stride does not depend on either.

Three routes and the bar of tests/test_gpu_epipolar.py:  e = max|x − ref64| / max|ref64|,  e_kernel <= max(4·e_torch32, 1e-6)."""
import pytest
import torch

from tests.epipolar_reference import epipolar_reference, make_case, margin_violations
from tests.test_gpu_epipolar import DEV, _err, _hold_to_the_bar, _run

pytestmark = pytest.mark.gpu

CASES = {"ragged": (235, 5, 7, (0, 117, 234)), "even": (33, 16, 16, (0, 16, 32))}
C, S = 3, 2
_CACHE = {}


def _big_case(name):
    b, h, w, _ = CASES[name]
    small = make_case(1, 2, h, w, C, S, 4000 + b)
    gen = torch.Generator().manual_seed(5000 + b)
    case = dict(small, images=torch.randn(b, 2, C, h, w, generator=gen, dtype=torch.float64))
    for k in ("extrinsics", "intrinsics", "near", "far"):
        case[k] = small[k].repeat(b, *([1] * (small[k].dim() - 1)))
    weights = torch.randn((b, 2, 1, h * w, S, C), generator=gen, dtype=torch.float64)
    return small, case, weights


def _element(case, weights, i):
    """batch element i of `case` as a b = 1 case of its own, with its slice of the loss weights"""
    one = {k: (v[i:i + 1] if torch.is_tensor(v) else v) for k, v in case.items()}
    return one, weights[i:i + 1]


def _routes(name):
    if name not in _CACHE:
        from ggrt_official_amd import fused_epipolar_sampler
        small, case, w = _big_case(name)
        ref = _run(epipolar_reference, case, torch.float64, "cpu", w)
        t32 = _run(epipolar_reference, case, torch.float32, DEV, w)
        ker = _run(fused_epipolar_sampler, case, torch.float32, DEV, w)
        alone = {}
        for i in CASES[name][3]:
            one, w_one = _element(case, w, i)
            alone[i] = _run(fused_epipolar_sampler, one, torch.float32, DEV, w_one)
        _CACHE[name] = (small, case, ref, t32, ker, alone)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_case_is_above_the_cap_and_admissible(name):
    b, h, w, elements = CASES[name]
    small, case, *_ = _routes(name)
    total = b * 2 * 1 * h * w
    assert total > 4096 * 4 and total - 4096 * 4 == {"ragged": 66, "even": 512}[name] and (total % 4 != 0) == (name == "ragged")
    # the last listed element holds second-trip pair-rays (p >= 16 384), the first none
    assert (elements[-1] + 1) * 2 * h * w > 4096 * 4 >= (elements[0] + 1) * 2 * h * w
    assert margin_violations(small) == 0
    for k in ("extrinsics", "intrinsics", "near", "far"):
        assert torch.equal(case[k][b - 1], small[k][0]) and torch.equal(case[k][b // 2], small[k][0]), k


@pytest.mark.parametrize("name", list(CASES))
def test_valid_outputs_and_gradient_match_the_float64_restatement_above_the_cap(name):
    """Reaches the loop's increment `p += gridDim.x * WAVES` (forward and backward) with p < total afterwards, which no case of
    tests/test_gpu_epipolar.py does (its largest has 858 pair-rays).  Smallest shape: see the module's docstring, 16 450 > 4096·4."""
    b, h, w, _ = CASES[name]
    _, case, ref, t32, ker, _ = _routes(name)
    assert ker["features"].shape == (b, 2, 1, h * w, S, C) and ker["valid"].shape == (b, 2, 1, h * w)
    assert bool(ref["valid"][b - 1].any())                # (the second-trip rays are not all invalid: their features are values, not zeros)
    _hold_to_the_bar(ref, t32, ker, f"above the cap, {name}: b={b} v=2 {h}x{w} c={C} s={S}")


@pytest.mark.parametrize("name", list(CASES))
def test_a_batch_element_equals_the_call_on_that_element_alone(name):
    """The forward is deterministic, so element i's outputs are the bits of a b = 1 call on element i's images: a pair-ray decoded to
    another camera or ray after the stride (`decode(a, p, R)` with the second trip's p) shows here.  dL/dimages is summed with
    float atomics, so it is held to the bar instead: the big call's and the single call's error against float64, on that element,
    each within max(4·e_torch32, 1e-6) of that element's float32 torch error."""
    b, h, w, elements = CASES[name]
    _, case, ref, t32, ker, alone = _routes(name)
    for i in elements:
        one = alone[i]
        for k in ("features", "valid", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions", "depth"):
            assert torch.equal(ker[k][i], one[k][0]), (name, i, k)
        r = ref["d_images"][i]
        e_big, e_one, e_t = _err(ker["d_images"][i], r), _err(one["d_images"][0], r), _err(t32["d_images"][i], r)
        print(f"{name} element {i:3d} d_images  e_kernel(b={b}) {e_big:.3e}  e_kernel(b=1) {e_one:.3e}  e_torch32 {e_t:.3e}")
        assert float(r.abs().max()) > 0 and e_big <= max(4 * e_t, 1e-6) and e_one <= max(4 * e_t, 1e-6), (name, i, e_big, e_one, e_t)
