"""The fused epipolar sampler's parallel-ray depth branch: `if (dot3(dir, dy) > 1.f - 1e-5f)` in `epipolar_fwd_kernel`
(csrc/epipolar.hip) — intersect_rays' "the rays are parallel: the point is 1e10".

Every other family of tests/epipolar_reference.py is kept at least 1e-4 away from that threshold on the non-parallel side by the
margin rule, so the branch never runs there.  The "rotation" family puts views 0 and 1 at the same point: a sample's ray of one is
the casting ray of the other up to rounding, the dot product is 1, and every sample of those pairs takes the branch; view 2 is
displaced, so the same launch holds non-parallel pairs too.  Sizes: 5×7 rays (35: not a multiple of a workgroup's four waves),
c = 4, v = 3 (the smallest with both kinds of pair), s = 1 and 8 (one lane and several in the depth's lane mask).

The contract on that branch: the point is (1e10, 1e10, 1e10), the distance |1e10 − origin| is far beyond `far` and is clipped to
it, and the relative disparity of `far` is 1 − (1/(far + 1e-10) − 1/(far + 1e-10))/(…) = 1: the same expression minus itself."""
import pytest
import torch

from tests.epipolar_reference import epipolar_reference, make_case, run_case
from tests.test_gpu_epipolar import _hold_to_the_bar, _routes

pytestmark = pytest.mark.gpu

B, V, H, W, C = 1, 3, 5, 7, 4


@pytest.mark.parametrize("s", [1, 8])
def test_two_views_that_differ_by_a_rotation_take_the_parallel_branch(s):
    case, ref, t32, ker = _routes(B, V, H, W, C, s, "rotation")
    shared = case["shared_centre"]
    assert shared.tolist() == [[True, False], [True, False], [False, False]]          # (0 → 1) and (1 → 0) share a centre
    det = run_case(epipolar_reference, case, details=True)
    low = run_case(epipolar_reference, case, torch.float32)
    # ---- the admissibility of the pair (view 0 casting, view 1 sampled), on the float64 restatement, before any kernel result is read
    pair = (0, 0, 0)
    for k in ("near_xy", "far_xy"):
        assert float(det[k][pair].min()) >= 0.02 and float(det[k][pair].max()) <= 0.98, k
    assert float(det["near_z"][pair].min()) > 0.1 and float(det["far_z"][pair].min()) > 0.1
    assert bool(det["min_valid"][pair].all()) and bool(det["max_valid"][pair].all())     # segments from the near and far projections
    assert bool(det["valid"][pair].all()) and bool(low["valid"][pair].all())
    assert float(det["dot"][pair].min()) > 1 - 1e-6
    # the reverse pair (view 1's wider frame cast into view 0): the rays that land inside view 0 are as parallel; the others are
    # invalid in float32 and in float64 alike (a frame intersection from the sampled camera's own centre is 0/0)
    back = (0, 1, 0)
    inside = det["valid"][back]
    assert bool(inside.any()) and not bool(inside.all()) and torch.equal(low["valid"], det["valid"])
    assert float(det["dot"][back][inside].min()) > 1 - 1e-6
    # and the pairs with view 2 are not parallel: both sides of the branch in one launch
    assert float(det["dot"][0, 2].max()) < 1 - 1e-5 - 1e-4 and float(det["dot"][0, 0, 1].max()) < 1 - 1e-5 - 1e-4

    _hold_to_the_bar(ref, t32, ker, f"rotation s={s} seed={case['seed']}")

    # ---- the depth of the branch, from the contract
    far = case["far"][0, :2].float().double()
    want = 1 - (1 / (far + 1e-10) - 1 / (far + 1e-10)) / (1 / (case["near"][0, :2].float().double() + 1e-10) - 1 / (far + 1e-10) + 1e-10)
    assert bool((want == 1).all())
    for view, rays in ((0, torch.ones(H * W, dtype=torch.bool)), (1, inside)):
        got = ker["depth"][0, view, 0][rays]
        assert got.shape == (int(rays.sum()), s)
        worst = float((got - want[view]).abs().max())
        print(f"rotation s={s} view {view}: {got.numel()} parallel samples, max |depth - 1| = {worst:.3e}")
        assert worst <= 2.0 ** -23, (view, worst)           # one float32 ulp of 1
        assert float((ref["depth"][0, view, 0][rays] - 1).abs().max()) == 0
