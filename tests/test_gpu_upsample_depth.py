"""`fused_upsample_depth` (csrc/upsample_depth.hip) on the GPU against the torch restatement of GGRt's `DepthPoseNet.upsample_depth`
with `disp_to_depth` (tests/upsample_depth_reference.py, pinned to the reference's own method by the fixtures).

Three routes: `ref` the restatement in float64 on the CPU, `t32` the restatement in float32 on the device, `ker` the kernels.
Buffers the launches must write whole are filled with NaN first.  The bar, every figure printed before it is asserted, for the value
and each of the two gradients: max |ker - ref| / max |ref| <= max(4 x the same figure of t32, 1e-6).  The bilinear weights are
continuous in the source coordinate, so no decision is injected and no pixel is excluded."""
import pytest
import torch
import torch.nn.functional as F

import ggrt_official_amd.splatting as splatting
from tests.test_upsample_depth_reference import DISP_RANGE, FULL_CASE, GPU_CASES, RESIZE_CASES
from tests.upsample_depth_reference import INPUTS, make_upsample_case, run_upsample_depth

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("out", "g_depth", "g_mask")


@pytest.fixture(autouse=True)
def _poison():
    splatting._IMAGE_LOSS_POISON = True
    yield
    splatting._IMAGE_LOSS_POISON = False


def _ker(*args, **kw):
    from ggrt_official_amd import fused_upsample_depth
    return fused_upsample_depth(*args, **kw)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a.reshape(b.shape) - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _check(name, case, **opts):
    ker = run_upsample_depth(_ker, case, torch.float32, DEV, **opts)
    ref = run_upsample_depth("torch", case, torch.float64, "cpu", **opts)
    t32 = run_upsample_depth("torch", case, torch.float32, DEV, **opts)
    for k in KEYS:
        assert ker[k] is not None and ker[k].dtype == torch.float32 and not torch.isnan(ker[k]).any(), k
        assert tuple(ker[k].shape) == tuple(ref[k].shape), (k, ker[k].shape, ref[k].shape)
        e32, e = _rel(t32[k], ref[k]), _rel(ker[k], ref[k])
        print(f"{name} {k}: kernel {e:.3e}, t32 {e32:.3e}")
        assert e <= max(4 * e32, 1e-6), (k, e, e32)
    return ref, t32, ker


@pytest.mark.parametrize("disp_range", [None, DISP_RANGE], ids=["plain", "disp"])
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_kernel_against_the_float64_restatement(name, disp_range):
    N, h, w, r, size, seed = GPU_CASES[name]
    _check(name, make_upsample_case(N, h, w, r, size, seed), ratio=r, image_size=size, disp_range=disp_range)


@pytest.mark.parametrize("disp_range", [None, DISP_RANGE], ids=["plain", "disp"])
@pytest.mark.parametrize("name", sorted(RESIZE_CASES))
def test_resize_regimes_against_the_float64_restatement(name, disp_range):
    """The backward gather's destination window (`reach()`) and the tile seams at the regimes tests/test_upsample_depth_reference.py
    names, plain and with the affine map.  The figures of the MI355X run: NOTES.md."""
    N, h, w, r, size, seed = RESIZE_CASES[name]
    _check(name, make_upsample_case(N, h, w, r, size, seed), ratio=r, image_size=size, disp_range=disp_range)


@pytest.mark.parametrize("disp_range", [None, DISP_RANGE], ids=["plain", "disp"])
def test_strong_down_leaves_the_unreached_pixels_exactly_zero(disp_range):
    """48 x 88 -> 3 x 5: an `up` pixel that no destination reaches (or reaches with weight 0 only) has dL/dmask exactly 0.0 for its
    nine taps, wherever the float32 restatement on the device — which forms the source coordinate as the kernel does — has.  `g` is
    in [0.5, 1.5], so a reached pixel has a nonzero gradient.  (That more than half is zero is a condition on the input, checked on
    the CPU too: tests/test_upsample_depth_reference.py.)"""
    N, h, w, r, size, seed = RESIZE_CASES["strong_down"]
    ref, t32, ker = _check("strong_down", make_upsample_case(N, h, w, r, size, seed), ratio=r, image_size=size, disp_range=disp_range)
    zero32 = (t32["g_mask"].reshape(N, 9, r * r, h, w) == 0).all(1, keepdim=True).expand(N, 9, r * r, h, w)
    got = ker["g_mask"].reshape(N, 9, r * r, h, w)
    share32, share = float((t32["g_mask"] == 0).double().mean()), float((got == 0).double().mean())
    print(f"strong_down: {share32:.4f} of t32's dL/dmask is exactly zero, {share:.4f} of the kernel's")
    assert share32 > 0.5
    assert bool((got[zero32] == 0).all()) and bool((got != 0).any())


def test_ggrt_shape():
    N, h, w, r, size, seed = FULL_CASE
    _check("ggrt_shape", make_upsample_case(N, h, w, r, size, seed), ratio=r, image_size=size, disp_range=DISP_RANGE)


@pytest.mark.parametrize("k", range(9))
def test_a_one_hot_mask_returns_the_zero_padded_neighbour_to_the_bit(k):
    """exp(0 - 200) underflows to exactly zero: p is one-hot and the convex sum is the tap itself."""
    N, h, w, r = 2, 4, 6, 4
    case = make_upsample_case(N, h, w, r, None, 930 + k)
    d = case["depth"].to(device=DEV, dtype=torch.float32)
    mask = torch.zeros(N, 9, r * r, h, w, device=DEV)
    mask[:, k] = 200.0
    out = _ker(d, mask.reshape(N, 9 * r * r, h, w), ratio=r)
    ky, kx = k // 3, k % 3
    want = F.pad(d, (1, 1, 1, 1))[:, :, ky:ky + h, kx:kx + w].repeat_interleave(r, 2).repeat_interleave(r, 3)
    assert torch.equal(out, want)


@pytest.mark.parametrize("shape", [(5, 7, (3, 4)), (5, 7, (40, 9)), (1, 6, (5, 6)), (64, 3, (2, 3)), (9, 9, (9, 9))], ids=lambda s: f"{s[0]}x{s[1]}_to_{s[2][0]}x{s[2][1]}")
def test_the_resize_is_a_linear_map_and_the_backward_its_adjoint(shape):
    """r = 1 and a one-hot mask on the centre tap (200 against 0: exact, as the one-hot test shows): the pass is
    F.interpolate(depth, size, bilinear, align_corners=True) and its transpose, so <out, g> = <depth, g_depth> up to rounding.  A
    destination the gather drops or counts twice breaks the identity by far more.  No restatement here: the bar is the same defect
    of float32 F.interpolate with autograd on the device, x 4, floor 1e-6; `out` against float64 F.interpolate under that bar too."""
    h, w, size = shape
    N, gen = 2, torch.Generator().manual_seed(950)
    depth64 = 0.05 + 0.9 * torch.rand(N, 1, h, w, generator=gen, dtype=torch.float64)
    g64 = torch.rand(N, 1, *size, generator=gen, dtype=torch.float64) + 0.5
    depth, g = depth64.to(device=DEV, dtype=torch.float32).requires_grad_(True), g64.to(device=DEV, dtype=torch.float32)
    mask = torch.zeros(N, 9, h, w, device=DEV)
    mask[:, 4] = 200.0
    out = _ker(depth, mask, ratio=1, image_size=size)
    g_depth, = torch.autograd.grad((out * g).sum(), depth)
    d32 = depth.detach().clone().requires_grad_(True)
    out32 = F.interpolate(d32, size=size, mode="bilinear", align_corners=True)
    g_depth32, = torch.autograd.grad((out32 * g).sum(), d32)
    assert out.shape == out32.shape and not torch.isnan(out).any() and not torch.isnan(g_depth).any()

    def defect(o, gd):
        lhs, rhs = (o.detach().double() * g.double()).sum(), (depth.detach().double() * gd.double()).sum()
        return float((lhs - rhs).abs() / lhs.abs())

    e, e32 = defect(out, g_depth), defect(out32, g_depth32)
    print(f"adjoint {h}x{w} -> {size}: kernel {e:.3e}, torch32 {e32:.3e}")
    assert e <= max(4 * e32, 1e-6), (e, e32)
    want = F.interpolate(depth64, size=size, mode="bilinear", align_corners=True)
    v, v32 = _rel(out, want), _rel(out32, want)
    print(f"resize {h}x{w} -> {size}: kernel {v:.3e}, torch32 {v32:.3e}")
    assert v <= max(4 * v32, 1e-6), (v, v32)


def test_an_all_zero_mask_is_the_zero_padded_box_mean():
    N, h, w, r = 2, 5, 7, 4
    case = make_upsample_case(N, h, w, r, None, 940)
    case["mask"] = torch.zeros_like(case["mask"])
    ref, t32, ker = _check("zero_mask", case, ratio=r)
    want = F.avg_pool2d(case["depth"], 3, 1, 1).repeat_interleave(r, 2).repeat_interleave(r, 3)
    e, e32 = _rel(ker["out"], want), _rel(t32["out"], want)
    print(f"zero_mask against avg_pool2d: kernel {e:.3e}, t32 {e32:.3e}")
    assert e <= max(4 * e32, 1e-6)
    ones = _ker(torch.ones(1, 1, h, w, device=DEV), torch.zeros(1, 9 * r * r, h, w, device=DEV), ratio=r).double().cpu()
    corners, edges, inner = ones[0, 0, [0, 0, -1, -1], [0, -1, 0, -1]], ones[0, 0, [0, -1, r, r], [r, r, 0, -1]], ones[0, 0, r:-r, r:-r]
    print(f"ones: corners {corners.tolist()}, edges {edges.tolist()}, interior {float(inner.min())} .. {float(inner.max())}")
    assert float((corners - 4 / 9).abs().max()) <= 1e-6 and float((edges - 6 / 9).abs().max()) <= 1e-6 and float((inner - 1).abs().max()) <= 1e-6


def test_large_logits_give_finite_values_and_gradients():
    N, h, w, r, size = 2, 5, 9, 8, (37, 70)
    case = make_upsample_case(N, h, w, r, size, 941)
    case["mask"] = 80.0 * torch.sign(case["mask"])
    for disp_range in (None, DISP_RANGE):
        ker = run_upsample_depth(_ker, case, torch.float32, DEV, ratio=r, image_size=size, disp_range=disp_range)
        for k in KEYS:
            assert bool(torch.isfinite(ker[k]).all()), k
    assert float(ker["g_depth"].abs().max()) > 0


_ROBUST = dict(N=3, h=5, w=13, r=4, size=(17, 55), seed=942)


@pytest.fixture(scope="module")
def robust():
    splatting._IMAGE_LOSS_POISON = True
    c = _ROBUST
    case = make_upsample_case(c["N"], c["h"], c["w"], c["r"], c["size"], c["seed"])
    opts = dict(ratio=c["r"], image_size=c["size"], disp_range=DISP_RANGE)
    return case, opts, run_upsample_depth(_ker, case, torch.float32, DEV, **opts)


def test_two_runs_give_the_same_bits(robust):
    case, opts, base = robust
    again = run_upsample_depth(_ker, case, torch.float32, DEV, **opts)
    for k in KEYS:
        assert torch.equal(base[k], again[k]), k


def test_a_list_input_equals_the_stacked_input(robust):
    case, opts, base = robust
    t = {k: v.to(device=DEV, dtype=torch.float32) for k, v in case.items()}
    depths = [t["depth"][n:n + 1].clone().requires_grad_(True) for n in range(3)]
    masks = [t["mask"][n:n + 1].clone().requires_grad_(True) for n in range(3)]
    out = _ker([depths[0], depths[1][:, 0], depths[2]], tuple(masks), **opts)          # ([1,1,h,w] and [1,h,w] maps)
    (out * t["g"]).sum().backward()
    assert torch.equal(out.detach(), base["out"])
    assert torch.equal(torch.cat([d.grad for d in depths]), base["g_depth"]) and torch.equal(torch.cat([m.grad for m in masks]), base["g_mask"])


def test_a_channels_last_mask_and_a_3d_depth(robust):
    case, opts, base = robust
    t = {k: v.to(device=DEV, dtype=torch.float32) for k, v in case.items()}
    mask = t["mask"].contiguous(memory_format=torch.channels_last).requires_grad_(True)
    depth = t["depth"].transpose(2, 3).contiguous().transpose(2, 3)[:, 0].requires_grad_(True)
    assert not mask.is_contiguous() and not depth.is_contiguous() and depth.dim() == 3
    out = _ker(depth, mask, **opts)
    (out * t["g"]).sum().backward()
    assert torch.equal(out.detach(), base["out"]) and torch.equal(mask.grad, base["g_mask"]) and torch.equal(depth.grad, base["g_depth"][:, 0])


@pytest.mark.parametrize("need", [("mask",), ("depth",), ()], ids=["mask", "depth", "nothing"])
def test_every_subset_of_requires_grad(robust, need):
    case, opts, base = robust
    got = run_upsample_depth(_ker, case, torch.float32, DEV, need=need, **opts)
    assert torch.equal(got["out"], base["out"])
    for k in INPUTS:
        if k in need:
            assert torch.equal(got["g_" + k], base["g_" + k]), k
        else:
            assert got["g_" + k] is None, k


def test_the_identity_size_equals_image_size_none():
    N, h, w, r = 2, 5, 9, 8
    case = make_upsample_case(N, h, w, r, None, 943)
    for disp_range in (None, DISP_RANGE):
        a = run_upsample_depth(_ker, case, torch.float32, DEV, ratio=r, image_size=None, disp_range=disp_range)
        b = run_upsample_depth(_ker, case, torch.float32, DEV, ratio=r, image_size=(r * h, r * w), disp_range=disp_range)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
    # ... and the plain one is torch's `up` through F.interpolate at that size, which is the identity to the bit
    t32 = run_upsample_depth("torch", case, torch.float32, DEV, need=(), ratio=r)
    assert torch.equal(F.interpolate(t32["out"], size=(r * h, r * w), mode="bilinear", align_corners=True), t32["out"])


def test_graph_replay_equals_eager():
    """Forward + backward captured on one stream, replayed with fresh inputs copied into the captured tensors."""
    N, h, w, r, size = 2, 5, 9, 8, (37, 70)
    first, second = make_upsample_case(N, h, w, r, size, 944), make_upsample_case(N, h, w, r, size, 945)
    opts = dict(ratio=r, image_size=size, disp_range=DISP_RANGE)
    eager = run_upsample_depth(_ker, second, torch.float32, DEV, **opts)
    t = {k: v.to(device=DEV, dtype=torch.float32) for k, v in first.items()}
    depth, mask, g = t["depth"].requires_grad_(True), t["mask"].requires_grad_(True), t["g"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # (warm-up on the side stream, as torch's graph recipe asks)
        for _ in range(2):
            torch.autograd.grad((_ker(depth, mask, **opts) * g).sum(), (depth, mask))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _ker(depth, mask, **opts)
        g_depth, g_mask = torch.autograd.grad((out * g).sum(), (depth, mask))
    with torch.no_grad():
        for k, dst in (("depth", depth), ("mask", mask), ("g", g)):
            dst.copy_(second[k].to(device=DEV, dtype=torch.float32))
    for buf in (out, g_depth, g_mask):
        buf.detach().fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager["out"]) and torch.equal(g_depth, eager["g_depth"]) and torch.equal(g_mask, eager["g_mask"])


def test_every_refusal():
    route = "DepthPoseNet.upsample_depth"
    mk = lambda N=2, h=3, w=4, r=8, c=None: (torch.zeros(N, 1, h, w, device=DEV), torch.zeros(N, 9 * r * r if c is None else c, h, w, device=DEV))
    for i, name in enumerate(("depth", "mask")):
        a = list(mk())
        a[i] = a[i].double()
        with pytest.raises(ValueError, match=name + " is torch.float64.*" + route):
            _ker(*a)
        a = list(mk())
        a[i] = a[i].cpu()
        with pytest.raises(ValueError, match=name + " is on cpu.*" + route):
            _ker(*a)
    with pytest.raises(ValueError, match="mask has 575 channels, not 9 \\* ratio\\^2 = 576.*" + route):
        _ker(*mk(c=575))
    with pytest.raises(ValueError, match="mask has 576 channels, not 9 \\* ratio\\^2 = 144.*" + route):
        _ker(*mk(), ratio=4)
    d, m = mk()
    with pytest.raises(ValueError, match="mask.*batch and spatial sizes.*" + route):
        _ker(d, m[:1])
    with pytest.raises(ValueError, match="mask.*batch and spatial sizes.*" + route):
        _ker(d, m[..., :3])
    with pytest.raises(ValueError, match="depth.*neither.*" + route):
        _ker(torch.zeros(2, 2, 3, 4, device=DEV), m)
    for ratio in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="ratio.*" + route):
            _ker(d, m, ratio=ratio)
    for size in ((0, 5), (5,), (4.0, 5), 7):
        with pytest.raises(ValueError, match="image_size.*" + route):
            _ker(d, m, image_size=size)
    for dr in ((0.0, 10.0), (2.0, 1.0), (1.0, 1.0), (1.0, float("inf")), (1.0,), 3.0):
        with pytest.raises(ValueError, match="disp_range.*" + route):
            _ker(d, m, disp_range=dr)
    with pytest.raises(ValueError, match="spatial sizes.*" + route):
        _ker([d, mk(h=4)[0]], [m, mk(h=4)[1]])
    assert _ker(d, m).shape == (2, 1, 24, 32) and _ker(d, m, image_size=(5, 6)).shape == (2, 1, 5, 6) and _ker(d[:, 0], m).shape == (2, 1, 24, 32)
