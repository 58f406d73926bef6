"""Inputs that the encoder passes' restatements define and no other GPU test feeds: a caller's `sh_mask` with zeros, a raw
quaternion of norm 0, saturated scale logits, one non-finite ray or pixel among finite ones, and empty calls.

Values are held to the project's bar against the float64 restatement: e = max|x − ref64| / max|ref64|,
e_kernel <= max(4·e_torch32, 1e-6).  Where a run is compared with another run of the same kernels, it is compared to the bit."""
import pytest
import torch

from tests import test_gpu_adapter as A
from tests import test_gpu_epipolar as E
from tests.adapter_reference import adapter_reference, make_case
from tests.encoder_cores import DEV, core_inputs, core_names, kernel_core, run_core_on

pytestmark = pytest.mark.gpu


def _adapter_routes(case, seed):
    from ggrt_official_amd import fused_gaussian_adapter
    w = A._weights(adapter_reference(**case), seed)
    return (A._run(adapter_reference, case, torch.float64, "cpu", w), A._run(adapter_reference, case, torch.float32, DEV, w),
            A._run(fused_gaussian_adapter, case, torch.float32, DEV, w))


@pytest.mark.parametrize("d_sh", [25, 4])
def test_a_callers_sh_mask_with_zeros(d_sh):
    """Reaches `dm[o + e] = T[…] * sh_mask[b + j]` and `msk[e] = sh_mask[e]` of `load_blocks` (csrc/adapter.hip) with a mask other
    than the built-in one, and `mj * row[…]` of the dL/dD accumulation with mj = 0: a kernel that ignored the argument, or applied
    the mask on the wrong side of D, differs in every higher band.  One zero in band 1 and one in the last band (for d_sh = 4 they
    are the same band); (C, G, spp) = (3, 255, 3): a ragged second tile, three samples per row."""
    case = make_case(3, 255, 3, d_sh, seed=300 + d_sh)
    mask = 0.25 + torch.rand(d_sh, generator=torch.Generator().manual_seed(301 + d_sh), dtype=torch.float64)
    mask[1] = 0.0
    mask[d_sh - 1] = 0.0
    case["sh_mask"] = mask
    ref, t32, ker = _adapter_routes(case, 300 + d_sh)
    assert float((ref["harmonics"] - adapter_reference(**dict(case, sh_mask=None))["harmonics"]).abs().max()) > 0.1
    raw_sh = ref["d_raw_gaussians"][..., 7:].reshape(3, 85, 3, d_sh)
    assert float(raw_sh[..., [1, d_sh - 1]].abs().max()) == 0 and float(ker["d_raw_gaussians"][..., 7:].reshape(3, 85, 3, d_sh)[..., [1, d_sh - 1]].abs().max()) == 0
    assert "d_sh_transform" in ref
    A._hold_to_the_bar(ref, t32, ker, f"caller's sh_mask d_sh={d_sh}")


def test_a_raw_quaternion_of_norm_zero():
    """Reaches `const float fall = nq > 0.f ? … : 0.f` of `adapter_bwd_kernel` on its second arm: |q| = 0 has the subgradient 0 in
    torch, so dL/dq = dn / eps (1e8 times the upstream's size) and the forward's quaternion is 0/eps = 0.  G = 130 is two full
    tiles and a ragged one of 2 rows; the zero rows sit at lane 0 (row 0), lane 63 (row 63) and in the ragged tile (row 129), one
    per camera.  Their dL/dq is held to the bar over those rows alone (at 1e8 it would drown every other row), everything else to the
    bar without them."""
    n_cam, g, d_sh = 3, 130, 4
    case = make_case(n_cam, g, 1, d_sh, seed=310)
    rows = [(0, 0), (1, 63), (2, 129)]
    for c, r in rows:
        case["raw_gaussians"][c, r, 3:7] = 0.0
    ref, t32, ker = _adapter_routes(case, 310)
    cam, row = torch.tensor([c for c, _ in rows]), torch.tensor([r for _, r in rows])
    for res in (ref, ker):
        assert float(res["rotations"].reshape(n_cam, g, 4)[cam, row].abs().max()) == 0
    at_zero = {k: {"d_q": v["d_raw_gaussians"][cam, row, 3:7]} for k, v in (("ref", ref), ("t32", t32), ("ker", ker))}
    assert float(at_zero["ref"]["d_q"].abs().max()) > 1e6 and bool(torch.isfinite(at_zero["ker"]["d_q"]).all())
    A._hold_to_the_bar(at_zero["ref"], at_zero["t32"], at_zero["ker"], "rows with |q| = 0")

    def without(res):
        res = {k: v.clone() for k, v in res.items()}
        res["d_raw_gaussians"][cam, row, 3:7] = 0.0
        return res
    A._hold_to_the_bar(without(ref), without(t32), without(ker), "the other rows")


def test_saturated_scale_logits():
    """`sigmoidf(±100)` of csrc/adapter.hip: 1/(1 + expf(−100)) = 1 and 1/(1 + expf(100)) = 1/inf = 0 in float32, so the scale is
    scale_max (scale_min) · depth · multiplier and `span * sg * (1 − sg)` is exactly 0.  In float64 sigmoid(100) rounds to 1
    (gradient exactly 0) and sigmoid(−100) = 3.7e-44 is still a number (gradient 3.7e-44 times the upstream: below 1e-40, zero to
    every purpose; asserted as such).  The scale's bound: the multiplier 0.1·Σ(K⁻¹·pixel) is seven float32 roundings (two
    reciprocals, the pixel size, the products, the sum, the constant and its product), the two products base·d·mult two more: 9
    half-ulps, held to 16·2^-24 = 2^-20 of the value computed in float64 from the float32 inputs."""
    n_cam, g, d_sh = 3, 130, 4
    case = make_case(n_cam, g, 1, d_sh, seed=320)
    hot = {(0, 0): (100.0, 100.0, 100.0), (1, 64): (-100.0, -100.0, -100.0), (2, 129): (100.0, -100.0, 100.0), (0, 63): (-100.0, 100.0, -100.0)}
    for (c, r), logits in hot.items():
        case["raw_gaussians"][c, r, :3] = torch.tensor(logits, dtype=torch.float64)
    ref, t32, ker = _adapter_routes(case, 320)
    K = case["intrinsics"].float().double()
    h, w = case["image_shape"]
    mult = 0.1 * (torch.linalg.inv(K[:, :2, :2]) @ torch.tensor([1.0 / w, 1.0 / h], dtype=torch.float64)).sum(-1)
    for (c, r), logits in hot.items():
        bound = torch.tensor([case["scale_max"] if x > 0 else case["scale_min"] for x in logits], dtype=torch.float64)
        want = bound * case["depths"][c, r].float().double() * mult[c]
        got = ker["scales"].reshape(n_cam, g, 3)[c, r]
        rel = float(((got - want).abs() / want).max())
        print(f"camera {c} row {r} logits {logits}: scales off by {rel:.3e} of the saturated value")
        assert rel <= 2.0 ** -20, (c, r, rel)
        assert float(ker["d_raw_gaussians"][c, r, :3].abs().max()) == 0
        g64 = ref["d_raw_gaussians"][c, r, :3]
        assert float(g64[torch.tensor(logits) > 0].abs().sum()) == 0 and float(g64.abs().max()) < 1e-40
    A._hold_to_the_bar(ref, t32, ker, "saturated logits")


@pytest.mark.parametrize("octaves", [None, 3])
def test_a_non_finite_ray_of_the_attention_cores_stays_in_its_ray(octaves):
    """A workgroup of `epipolar_attn_*_kernel` / `epipolar_attn_enc_*_kernel` owns one ray (`n = blockIdx.x`) and shares nothing:
    NaN in ray 1's samples and +inf in ray 3's query must leave rays 0, 2, 4 with the bits of a call on those three alone, forward
    and backward.  S = 33, C = 20, H = 3 as the cores' own row tests."""
    encoded = octaves is not None
    t = core_inputs(5, 33, 20, 3, 330 + (octaves or 0), octaves)
    f32 = lambda x: x.to(device=DEV, dtype=torch.float32)
    leaves = [f32(t[k]) for k in (("qk", "qe", "f", "d") if encoded else ("qk", "z"))]
    grads = [f32(t[k]) for k in (("g_ctx_f", "g_ctx_e") if encoded else ("g_ctx",))]
    leaves[2 if encoded else 1][1, 7, 5] = float("nan")
    leaves[0][3, 1, 2] = float("inf")
    keep = torch.tensor([0, 2, 4], device=DEV)
    fn = kernel_core(encoded)
    whole = run_core_on(fn, leaves, grads)
    three = run_core_on(fn, [x[keep].contiguous() for x in leaves], [x[keep].contiguous() for x in grads])
    for name, a, b in zip(core_names(encoded), whole, three):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0, name
        assert torch.equal(a[keep], b), name
    assert not bool(torch.isfinite(whole[0][1]).all()) and not bool(torch.isfinite(whole[0][3]).all())      # (and the two rays do carry it)


def test_a_nan_pixel_reaches_only_the_pair_rays_that_tap_it():
    """One NaN at (view 1, channel 2, y 5, x 6) of 11×13 maps, v = 3: `map[t.at[k] * c + ch] * t.w[k]` of `epipolar_fwd_kernel`
    reads it only for the samples with a tap on that pixel.  Which pair-rays those are comes from the CLEAN run's xy_sample, taken
    generously (a tap within 1e-3 of the pixel's neighbourhood counts as touching); every other pair-ray's features are the clean
    run's bits.  dL/dimages does not depend on the maps' values at all (the gather is linear in them), so it is held to the bar
    against the clean float64 gradient everywhere."""
    from ggrt_official_amd import fused_epipolar_sampler
    b, v, h, w, c, s = 1, 3, 11, 13, 4, 8
    case, ref, t32, clean = E._routes(b, v, h, w, c, s)
    seed = 3 * b + 5 * v + 7 * h + 11 * w + 13 * c + 17 * s
    images = case["images"].clone()
    images[0, 1, 2, 5, 6] = float("nan")
    dirty = E._run(fused_epipolar_sampler, dict(case, images=images), torch.float32, DEV, E._weights(case, seed))
    ix, iy = clean["xy_sample"][..., 0] * w - 0.5, clean["xy_sample"][..., 1] * h - 0.5
    near_pixel = ((ix - 6).abs() < 1 + 1e-3) & ((iy - 5).abs() < 1 + 1e-3)                      # [b, v, v-1, r, s]
    from tests.epipolar_reference import other_views
    samples_view_1 = (other_views(v) == 1)[None, :, :, None]
    touched = (near_pixel.any(-1) & samples_view_1 & clean["valid"])                             # [b, v, v-1, r]
    assert 0 < int(touched.sum()) < int(clean["valid"].sum()) // 2
    assert bool(dirty["features"][touched].isnan().any()) and torch.equal(dirty["valid"], clean["valid"])
    assert torch.equal(dirty["features"][~touched], clean["features"][~touched])
    assert bool(torch.isfinite(dirty["features"][..., [0, 1, 3]]).all())                         # (the other channels never see it)
    for k in ("xy_sample", "depth", "origins", "directions"):
        assert torch.equal(dirty[k], clean[k]), k
    assert bool(torch.isfinite(dirty["d_images"]).all())
    e_k, e_t = E._err(dirty["d_images"], ref["d_images"]), E._err(t32["d_images"], ref["d_images"])
    print(f"NaN pixel: d_images e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
    assert e_k <= max(4 * e_t, 1e-6)


def test_empty_adapter_calls():
    """No cameras: empty outputs of the right shapes and empty gradients, no launch (`ggr_adapter_forward` returns before it).
    Cameras without Gaussians: `raw_gaussians` has no rows to share, which the wrapper refuses with a ValueError."""
    from ggrt_official_amd import fused_gaussian_adapter
    case = make_case(2, 12, 3, 4, seed=340)
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    none = {k: (v[:0].clone().requires_grad_(True) if torch.is_tensor(v) else v) for k, v in args.items()}
    out = fused_gaussian_adapter(**none)
    assert out.means.shape == (0, 3) and out.scales.shape == (0, 3) and out.rotations.shape == (0, 4) and out.harmonics.shape == (0, 3, 4)
    leaves = [none[k] for k in A.LEAVES]
    grads = torch.autograd.grad(out.means.sum() + out.scales.sum() + out.rotations.sum() + out.harmonics.sum(), leaves, allow_unused=True)
    for k, leaf, g in zip(A.LEAVES, leaves, grads):
        assert g is None or (g.shape == leaf.shape and g.numel() == 0), k
    with pytest.raises(ValueError):
        fused_gaussian_adapter(**dict(args, coordinates=args["coordinates"][:, :0], depths=args["depths"][:, :0],
                                      raw_gaussians=args["raw_gaussians"][:, :0]))


@pytest.mark.parametrize("octaves", [None, 3])
def test_empty_attention_calls(octaves):
    """N = 0: empty outputs of the right shapes and empty gradients (`ggr_epipolar_attention*_forward` returns before the launch)"""
    encoded = octaves is not None
    t = core_inputs(2, 9, 7, 3, 350, octaves)
    f32 = lambda x: x[:0].to(device=DEV, dtype=torch.float32)
    leaves = [f32(t[k]) for k in (("qk", "qe", "f", "d") if encoded else ("qk", "z"))]
    grads = [f32(t[k]) for k in (("g_ctx_f", "g_ctx_e") if encoded else ("g_ctx",))]
    got = dict(zip(core_names(encoded), run_core_on(kernel_core(encoded), leaves, grads)))
    want = dict(ctx_f=(0, 3, 7), ctx_e=(0, 3, 6), attn=(0, 3, 9), g_qk=(0, 3, 7), g_qe=(0, 3, 6), g_f=(0, 9, 7), g_d=(0, 9)) if encoded else \
        dict(ctx=(0, 3, 7), attn=(0, 3, 9), g_qk=(0, 3, 7), g_z=(0, 9, 7))
    assert {k: tuple(v.shape) for k, v in got.items()} == want
