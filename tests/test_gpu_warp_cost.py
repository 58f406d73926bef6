"""`fused_warp_cost` (csrc/warp_cost.hip) on the GPU against the torch restatement of GGRt's `DepthPoseNet.get_cost_each` /
`depth_cost_calc` (tests/warp_cost_reference.py, pinned to the reference's own methods by the fixtures).

Three routes: `ref` the restatement in float64 on the CPU, `t32` the restatement in float32 on the device, `ker` the kernels.  Both
restatements receive the kernel's own `cells` (bilinear cell and P.z-clamp flag) through `decisions=`, so a pixel whose coordinate
sits within rounding of a cell border is compared like any other: nothing is excluded.  Buffers the launches must write whole are
filled with NaN first.  The bar, every figure printed before it is asserted, for the cost and each of the four gradients:
max |ker - ref| / max |ref| <= max(4 x the same figure of t32, 1e-6).  The inputs' condition — under 2 % of the (view, pixel) pairs
within 8 x the float32 coordinate error of a border — is measured on the CPU for every case but the identity one (also checked
without a GPU by tests/test_warp_cost_reference.py)."""
import itertools

import pytest
import torch

import ggrt_official_amd.splatting as splatting
from tests.test_warp_cost_reference import FULL_CASE, GPU_CASES
from tests.warp_cost_reference import INPUTS, make_warp_case, near_border_share, run_warp_cost

pytestmark = pytest.mark.gpu
DEV = "cuda"
# dL/dfmaps_ref between two runs, or two subsets of requires_grad: the same terms in another order.  An element receives a tap from
# each pixel whose sample falls in one of its four cells — at these poses a handful, never more than 16 — so the orders differ by at
# most 16 x 2^-24 of the sum of the terms' magnitudes, which the element's own scale bounds up to the cancellation between terms;
# held against the tensor's maximum: 4e-6.  This covers the moderate-pose cases only; where every sample lands in one cell
# (test_scatter_into_one_cell) the bar is derived there, per element
ORDER_BAR = 4e-6


@pytest.fixture(autouse=True)
def _poison():
    splatting._IMAGE_LOSS_POISON = True
    yield
    splatting._IMAGE_LOSS_POISON = False


def _ker(*args, **kw):
    from ggrt_official_amd import fused_warp_cost
    return fused_warp_cost(*args, **kw)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a.reshape(b.shape) - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _check(name, case, form, s, disp_range=None, keys=("cost",) + tuple("g_" + k for k in INPUTS), condition=True):
    kw = dict(reduce=form, scale_factor=s, disp_range=disp_range)
    ker = run_warp_cost(_ker, case, torch.float32, DEV, **kw)
    cells = ker["cells"].cpu()
    V, h, w = cells.shape[:3]
    assert cells.dtype == torch.int32 and tuple(cells.shape) == (V, h, w, 3) and int(cells.min()) >= -2 and int(cells[..., 2].max()) <= 1
    if condition:
        own64 = run_warp_cost("torch", case, torch.float64, "cpu", need=(), **kw)
        own32 = run_warp_cost("torch", case, torch.float32, "cpu", need=(), **kw)
        share, e, ez = near_border_share(own64, own32, h, w)
        differ = float((cells != own64["cells"]).any(-1).double().mean())
        print(f"{name}: coordinate error {e:.3e}, near-border share {share:.4%}, cells that differ from float64's own {differ:.4%}")
        assert share < 0.02 and differ < 0.02
    ref = run_warp_cost("torch", case, torch.float64, "cpu", decisions=cells, **kw)
    t32 = run_warp_cost("torch", case, torch.float32, DEV, decisions=cells.to(DEV), **kw)
    for k in keys:
        assert ker[k] is not None and not torch.isnan(ker[k]).any(), k
        assert tuple(ker[k].shape) == tuple(ref[k].shape), (k, ker[k].shape, ref[k].shape)
        if float(ref[k].abs().max()) == 0:
            assert float(ker[k].abs().max()) == 0, k
            continue
        e32, e = _rel(t32[k], ref[k]), _rel(ker[k], ref[k])
        print(f"{name} {k}: kernel {e:.3e}, t32 {e32:.3e}")
        assert e <= max(4 * e32, 1e-6), (k, e, e32)
    return ref, t32, ker


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_kernel_against_the_float64_restatement(name):
    V, C, h, w, seed, s, form, opts = GPU_CASES[name]
    _check(name, make_warp_case(V, C, h, w, seed, scale_factor=s, **opts), form, s, opts.get("disp_range"))


@pytest.mark.parametrize("form", ["mean", "none"])
def test_ggrt_shape(form):
    V, C, h, w, seed, s = FULL_CASE
    _check("ggrt_shape_" + form, make_warp_case(V, C, h, w, seed, scale_factor=s), form, s)


@pytest.mark.parametrize("s", [1.0, 1.0 / 8])
def test_identity_pose_with_equal_intrinsics(s):
    """u = x and v = y exactly: the warped map IS the reference map, cost = (fmap - fmaps_ref)^2 to the bit.  Every coordinate sits on
    an integer, so only the values and the gradients to the two maps are compared."""
    case = make_warp_case(2, 5, 9, 13, 840, scale_factor=s, identity=True)
    ref, t32, ker = _check("identity", case, "none", s, keys=("cost", "g_fmap", "g_fmaps_ref"), condition=False)
    closed = (case["fmap"].float() - case["fmaps_ref"].float()) ** 2
    assert torch.equal(ker["cost"].cpu(), closed)
    cells = ker["cells"].cpu()
    ys, xs = torch.meshgrid(torch.arange(9), torch.arange(13), indexing="ij")
    assert bool((cells[..., 0] == xs).all() and (cells[..., 1] == ys).all() and (cells[..., 2] == 0).all())


def test_a_view_wholly_out_of_frame():
    case = make_warp_case(3, 4, 9, 12, 841, far_view=1)
    for form in ("none", "mean"):
        ref, t32, ker = _check("far_view_" + form, case, form, 1.0 / 8)
        assert bool((ker["cells"][1, ..., :2] == -2).all())
        assert float(ker["g_poses"][1].abs().max()) == 0 and float(ker["g_fmaps_ref"][1].abs().max()) == 0
        assert float(ker["g_poses"][0].abs().max()) > 0 and float(ker["g_fmaps_ref"][2].abs().max()) > 0
        if form == "none":
            assert torch.equal(ker["cost"][1].cpu(), (case["fmap"].float()[0]) ** 2)


def test_points_behind_the_reference_camera_set_the_clamp_flag():
    case = make_warp_case(2, 3, 9, 12, 842, behind_view=0)
    ref, t32, ker = _check("behind", case, "none", 1.0 / 8)
    assert bool((ker["cells"][0, ..., 2] == 1).all() and (ker["cells"][1, ..., 2] == 0).all())
    assert float((ref["pz"][0]).max()) < 0
    assert torch.equal(ker["cost"][0].cpu(), (case["fmap"].float()[0]) ** 2) and float(ker["g_poses"][0].abs().max()) == 0


def test_a_block_of_nonpositive_inverse_depth_gets_no_gradient():
    V, C, h, w, seed, s, form, opts = GPU_CASES["nonpositive_block"]
    case = make_warp_case(V, C, h, w, seed, scale_factor=s, **opts)
    assert float(case["inv_depth"][0, 0, 0, 0]) < 0 and float(case["inv_depth"][0, 0, 1, 1]) == 0
    ker = run_warp_cost(_ker, case, torch.float32, DEV, reduce=form, scale_factor=s)
    block = ker["g_inv_depth"][0, 0, : h // 3, : w // 3]
    assert float(block.abs().max()) == 0 and float(ker["g_inv_depth"].abs().max()) > 0


_SUBSET_CASE = dict(V=2, C=9, h=5, w=13, seed=843)


@pytest.fixture(scope="module")
def subset_full():
    splatting._IMAGE_LOSS_POISON = True
    case = make_warp_case(**_SUBSET_CASE)
    return case, run_warp_cost(_ker, case, torch.float32, DEV, reduce="mean")


@pytest.mark.parametrize("need", [c for r in range(5) for c in itertools.combinations(INPUTS, r)], ids=lambda c: "+".join(c) or "nothing")
def test_every_subset_of_requires_grad(subset_full, need):
    case, full = subset_full
    got = run_warp_cost(_ker, case, torch.float32, DEV, need=need, reduce="mean")
    assert torch.equal(got["cost"], full["cost"])
    for k in INPUTS:
        if k not in need:
            assert got["g_" + k] is None, k
        elif k == "fmaps_ref":
            assert float((got["g_" + k] - full["g_" + k]).abs().max()) <= ORDER_BAR * float(full["g_" + k].abs().max())
        else:
            assert torch.equal(got["g_" + k], full["g_" + k]), k


def test_two_runs_give_the_same_bits():
    case = make_warp_case(5, 33, 9, 15, 844)
    for form in ("mean", "none"):
        a = run_warp_cost(_ker, case, torch.float32, DEV, reduce=form)
        b = run_warp_cost(_ker, case, torch.float32, DEV, reduce=form)
        for k in ("cost", "cells", "g_fmap", "g_inv_depth", "g_poses"):
            assert torch.equal(a[k], b[k]), (form, k)
        assert float((a["g_fmaps_ref"] - b["g_fmaps_ref"]).abs().max()) <= ORDER_BAR * float(a["g_fmaps_ref"].abs().max())


def _gpu_case(name):
    V, C, h, w, seed, s, form, opts = GPU_CASES[name]
    return make_warp_case(V, C, h, w, seed, scale_factor=s, **opts), dict(reduce=form, scale_factor=s, disp_range=opts.get("disp_range"))


def _views(case, lo, hi):
    return {k: (v[lo:hi] if k in ("fmaps_ref", "ref_Ks", "poses", "g_none") else v) for k, v in case.items()}


def test_views_8_to_15_of_16_alone_give_the_same_bits():
    """In the "none" form the views are independent: rows 8..15 of the tile's coordinate table and of the cameras, which only a
    second trip of `tile_coordinates` fills, must hold what rows 0..7 hold when those views come alone."""
    case, kw = _gpu_case("v16_none")
    full = run_warp_cost(_ker, case, torch.float32, DEV, **kw)
    half = run_warp_cost(_ker, _views(case, 8, 16), torch.float32, DEV, **kw)
    for k in ("cost", "cells", "g_poses"):
        assert tuple(half[k].shape[1:]) == tuple(full[k].shape[1:]) and half[k].shape[0] == 8
        assert torch.equal(full[k][8:], half[k]), k
    assert float(half["g_poses"].abs().amax(1).min()) > 0 and int((half["cells"][..., 0] >= 0).flatten(1).sum(1).min()) > 0


def test_tiles_beyond_the_pose_kernels_first_trip():
    """130 tiles: dL/dposes is the same bits twice, and with the upstream gradient zeroed on the first 64 tiles, so that nothing but
    the pose kernel's second and third strided trips (the last a tail of two tiles, one of them partial) contributes, it still meets
    the bar and is not zero."""
    from tests.test_warp_cost_reference import upstream_beyond_tile_63
    case, kw = _gpu_case("tiles130_tail")
    a, b = (run_warp_cost(_ker, case, torch.float32, DEV, need=("poses",), **kw) for _ in range(2))
    assert torch.equal(a["g_poses"], b["g_poses"]) and float(a["g_poses"].abs().amax(1).min()) > 0
    masked = upstream_beyond_tile_63(case)
    ref, t32, ker = _check("tiles130_tail_beyond_tile_63", masked, kw["reduce"], kw["scale_factor"])
    assert float(ker["g_poses"].abs().amax(1).min()) > 0 and float(ker["g_fmap"].flatten(2)[..., :4096].abs().max()) == 0
    assert not torch.equal(ker["g_poses"], a["g_poses"])


def test_a_view_that_straddles_the_clamp_inside_a_tile():
    case, kw = _gpu_case("straddle")
    ref, t32, ker = _check("straddle", case, kw["reduce"], kw["scale_factor"])
    flag = ker["cells"][0, ..., 2].cpu() == 1
    assert bool(flag.flatten()[:64].any()) and bool((~flag).flatten()[:64].any()) and bool((ker["cells"][1, ..., 2] == 0).all())
    # behind the camera Z is the constant 1e-5 and the sample leaves the frame: the cost is fmap^2 and view 0 adds nothing to the
    # pixel's dL/dinv_depth, which the kernel sums over the views in a register in their order — view 1 alone gives the same bits
    assert bool((ker["cells"][0, ..., :2].cpu()[flag] == -2).all())
    assert torch.equal(ker["cost"][0].cpu()[:, flag], (case["fmap"].float()[0] ** 2)[:, flag])
    alone = run_warp_cost(_ker, _views(case, 1, 2), torch.float32, DEV, **kw)
    assert torch.equal(ker["g_inv_depth"][0, 0].cpu()[flag], alone["g_inv_depth"][0, 0].cpu()[flag])
    assert float(alone["g_inv_depth"][0, 0].cpu()[flag].abs().max()) > 0
    assert not torch.equal(ker["g_inv_depth"][0, 0].cpu()[~flag], alone["g_inv_depth"][0, 0].cpu()[~flag])


@pytest.mark.parametrize("name", ["depth_column", "depth_column_disp"])
def test_the_inverse_depth_gate_row_by_row(name):
    """Every sample of the column is in frame (checked on the CPU), so a zero in dL/dinv_depth is the gate's doing: exactly zero where
    the depth is a constant (d = 1e-7 under the clamp, 0, -1), not zero where it is 1 / d (just above 1e-6, and 1e3).  The row at the
    gate itself (plain: d = 1e-6 exactly; folded: the same number as the row above it, see `_raw_disparity`) is held against the
    restatement by `_check` like every other element, and takes the restatement's side."""
    from tests.warp_cost_reference import DEPTH_COLUMN_VALUES
    case, kw = _gpu_case(name)
    x = GPU_CASES[name][7]["depth_column"]
    ref, t32, ker = _check(name, case, kw["reduce"], kw["scale_factor"], kw["disp_range"])
    col, col64 = ker["g_inv_depth"][0, 0, :, x].cpu(), ref["g_inv_depth"][0, 0, :, x]
    print(f"{name}: dL/dinv_depth down the column, kernel {col.tolist()}, float64 {col64.tolist()}")
    assert DEPTH_COLUMN_VALUES[0] == 1e-7 and DEPTH_COLUMN_VALUES[4:] == (0.0, -1.0) and DEPTH_COLUMN_VALUES[2:4] == (1.0000001e-6, 1e3)
    assert bool((col[[0, 4, 5]] == 0).all()) and bool((col[[2, 3]] != 0).all())
    assert (float(col[1]) != 0) == (float(col64[1]) != 0)
    assert bool((ker["cells"][:, :, x, :2] != -2).all())


def test_scatter_into_one_cell():
    """Every pixel's sample lands in one cell: 128 float atomics on each of four addresses per channel.  The case is built so that
    all terms of one element have the same sign; summing 128 such float32 terms in any order is within 127 x 2^-24 of the sum."""
    from tests.test_warp_cost_reference import COLLAPSE_CASE
    V, C, h, w, seed, s = COLLAPSE_CASE
    case = make_warp_case(V, C, h, w, seed, scale_factor=s, collapse=True)
    ref, t32, ker = _check("collapse", case, "none", s, keys=("cost", "g_fmap", "g_inv_depth", "g_poses"))
    cells = ker["cells"].cpu()
    assert bool((cells == torch.tensor([w // 2, h // 2, 0], dtype=torch.int32)).all())
    hit = torch.zeros(h, w, dtype=torch.bool)
    hit[h // 2: h // 2 + 2, w // 2: w // 2 + 2] = True
    again = run_warp_cost(_ker, case, torch.float32, DEV, need=("fmaps_ref",), reduce="none", scale_factor=s)
    g, g2, g32, g64 = (r["g_fmaps_ref"][0].double().cpu() for r in (ker, again, t32, ref))
    assert not torch.isnan(g).any() and bool((g[:, hit] != 0).all()) and bool((g[:, ~hit] == 0).all()) and bool((g2[:, ~hit] == 0).all())
    bar = torch.maximum(4 * (g32 - g64).abs(), 127 * 2.0 ** -24 * g64.abs())[:, hit]
    e, e2 = (g - g64).abs()[:, hit], (g - g2).abs()[:, hit]
    print(f"collapse g_fmaps_ref, per element over |ref|: kernel {(e / g64[:, hit].abs()).tolist()}, t32 {((g32 - g64).abs()[:, hit] / g64[:, hit].abs()).tolist()}, "
          f"two runs {(e2 / g64[:, hit].abs()).tolist()}; 127 x 2^-24 = {127 * 2.0 ** -24:.3e}")
    assert bool((e <= bar).all()) and bool((e2 <= bar).all())


def test_list_inputs_and_noncontiguous_inputs():
    case = make_warp_case(3, 5, 7, 9, 845)
    base = run_warp_cost(_ker, case, torch.float32, DEV, reduce="none")
    t = {k: v.to(device=DEV, dtype=torch.float32) for k, v in case.items()}
    fmap = t["fmap"].clone().requires_grad_(True)
    refs = [t["fmaps_ref"][j:j + 1].clone().requires_grad_(True) for j in range(3)]
    poses = [t["poses"][j:j + 1].clone().requires_grad_(True) for j in range(3)]
    inv = t["inv_depth"].clone().requires_grad_(True)
    cost = _ker(fmap, tuple(refs), inv, t["K"][0], t["ref_Ks"], poses, reduce="none")
    (cost * t["g_none"]).sum().backward()
    assert torch.equal(cost.detach(), base["cost"]) and torch.equal(fmap.grad, base["g_fmap"]) and torch.equal(inv.grad, base["g_inv_depth"])
    assert torch.equal(torch.cat([p.grad for p in poses]), base["g_poses"])
    assert float((torch.cat([r.grad for r in refs]) - base["g_fmaps_ref"]).abs().max()) <= ORDER_BAR * float(base["g_fmaps_ref"].abs().max())
    # non-contiguous views of every input: a channels-last map, a transposed stack, strided intrinsics and poses
    fmap_nc = t["fmap"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    refs_nc = t["fmaps_ref"].transpose(2, 3).contiguous().transpose(2, 3)
    inv_nc = t["inv_depth"].transpose(2, 3).contiguous().transpose(2, 3)
    K_nc = torch.stack([t["K"], t["K"]], -1)[..., 0]
    Ks_nc = torch.stack([t["ref_Ks"], t["ref_Ks"]], -1)[..., 1]
    poses_nc = torch.cat([t["poses"], t["poses"]], 1)[:, :6].requires_grad_(True)
    assert not (fmap_nc.is_contiguous() or refs_nc.is_contiguous() or inv_nc.is_contiguous() or K_nc.is_contiguous() or Ks_nc.is_contiguous() or poses_nc.is_contiguous())
    cost = _ker(fmap_nc, refs_nc, inv_nc, K_nc, Ks_nc, poses_nc, reduce="none")
    (cost * t["g_none"]).sum().backward()
    assert torch.equal(cost.detach(), base["cost"]) and torch.equal(fmap_nc.grad, base["g_fmap"]) and torch.equal(poses_nc.grad, base["g_poses"])


def test_every_refusal():
    V, C, h, w = 2, 3, 4, 5
    def mk(V=V, C=C, h=h, w=w, B=1):
        return [torch.zeros(B, C, h, w, device=DEV), torch.zeros(V, C, h, w, device=DEV), torch.ones(B, 1, h, w, device=DEV),
                torch.eye(3, device=DEV)[None], torch.eye(3, device=DEV).repeat(V, 1, 1), torch.zeros(V, 6, device=DEV)]
    route = "get_cost_each"
    names = ("fmap", "fmaps_ref", "inv_depth", "K", "ref_Ks", "poses")
    for i, name in enumerate(names):
        a = mk()
        a[i] = a[i].double()
        with pytest.raises(ValueError, match=name + " is torch.float64.*" + route):
            _ker(*a)
        a = mk()
        a[i] = a[i].cpu()
        with pytest.raises(ValueError, match=name + " is on cpu.*" + route):
            _ker(*a)
    a = mk()
    a[1] = torch.zeros(V, C, h, w + 1, device=DEV)
    with pytest.raises(ValueError, match="fmaps_ref.*spatial sizes.*" + route):
        _ker(*a)
    a = mk()
    a[2] = torch.ones(1, 1, h + 1, w, device=DEV)
    with pytest.raises(ValueError, match="inv_depth.*spatial sizes.*" + route):
        _ker(*a)
    with pytest.raises(ValueError, match="fmap.*below 2 x 2.*" + route):
        _ker(*mk(h=1))
    with pytest.raises(ValueError, match="fmap.*below 2 x 2.*" + route):
        _ker(*mk(w=1))
    with pytest.raises(ValueError, match=r"fmaps_ref.*V = 0.*" + route):
        _ker(*mk(V=0))
    a = mk()
    a[1] = []
    with pytest.raises(ValueError, match=r"fmaps_ref.*V = 0.*" + route):
        _ker(*a)
    with pytest.raises(ValueError, match="fmaps_ref holds 17 views.*" + route):
        _ker(*mk(V=17))
    with pytest.raises(ValueError, match="fmap.*batch other than 1.*" + route):
        _ker(*mk(B=2))
    a = mk()
    a[2] = torch.ones(2, 1, h, w, device=DEV)
    with pytest.raises(ValueError, match="inv_depth.*batch other than 1.*" + route):
        _ker(*a)
    a = mk()
    a[1] = [torch.zeros(2, C, h, w, device=DEV)]
    with pytest.raises(ValueError, match="fmaps_ref.*batch other than 1.*" + route):
        _ker(*a)
    for s in (0.0, -0.125, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale_factor.*" + route):
            _ker(*mk(), scale_factor=s)
    with pytest.raises(ValueError, match="reduce 'sum'.*" + route):
        _ker(*mk(), reduce="sum")
    for dr in ((0.0, 10.0), (2.0, 1.0), (1.0, 1.0), (-1.0, 2.0), (1.0, float("inf")), (1.0,), 3.0):
        with pytest.raises(ValueError, match="disp_range.*" + route):
            _ker(*mk(), disp_range=dr)
    for i in (3, 4):
        a = mk()
        a[i].requires_grad_(True)
        with pytest.raises(RuntimeError, match=names[i] + " requires grad"):
            _ker(*a)
    assert _ker(*mk(V=16)).shape == (1, C, h, w) and _ker(*mk(), reduce="none").shape == (V, C, h, w)
