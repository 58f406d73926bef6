"""The fused depth head (csrc/depth_head.hip, `fused_depth_head`) against its float64 restatement (tests/depth_head_reference.py),
forward and backward.

`index` must equal the float64 restatement's on EVERY row (the inputs obey the index-margin rule of `make_case`).  For every float
output and every gradient (dL/dlogits, dL/dxy_raw)  e = max|x − ref64| / max|ref64|;  `e_kernel` is the kernels', `e_torch32` the
restatement's run in float32 on the device.  The bar:  e_kernel <= max(4·e_torch32, 1e-6).  The loss is Σ over depths, opacities
and coordinates of (output · fixed random weights).

Shapes: the smallest at which the kernels can go wrong.  A tile is 64 heads (ray × surface) and a workgroup one wave (64 lanes),
so R·srf = 1, 63, 64, 65, 257 are below / at / above a tile and five tiles; three cameras put a camera boundary next to a ragged
tile; srf = 2 interleaves two heads in a ray's row and srf = 3 makes tiles end inside a ray (64 is no multiple of 3); spp = 1, 2, 3,
5, 16 take the kernels instantiated for 1, 2, 4, 8, 16 samples; s = 1, 2, 31, 32, 33, 64 walk the bucket loops and the LDS pitch;
R = 44801 at three cameras is beyond 2048/3 workgroups per camera, where a workgroup strides over several tiles.

use_transmittance is never paired with opacity_exponent < 1 where gradients are compared: at the last bucket the transmittance
form is q = pdf/(1 − Σ_{d<last} pdf + 1e-10) = 1 up to rounding, and d/dq (1 − q)^e = e·(1 − q)^(e−1) is singular there for e < 1 —
about 1e5 in float64 and inf or NaN in any float32 route, the torch one included (first seen at s = 2: e_kernel = e_torch32 = nan).
Exponents 1 and 2**0.5 go with the transmittance form, 2**-1 with the plain one; the FORWARD of the transmittance form at 2**-1
has a test of its own."""
import pytest
import torch

from tests.depth_head_reference import depth_head_reference, make_case, margin_violations

pytestmark = pytest.mark.gpu

OUTPUTS = ("depths", "opacities", "coordinates")
LEAVES = ("logits", "xy_raw")
DEV = "cuda:0"


def _as_dict(out):
    return out if isinstance(out, dict) else dict(depths=out.depths, opacities=out.opacities, coordinates=out.coordinates, index=out.index)


def _weights(case, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    n_cam, rays = case["logits"].shape[:2]
    g = rays * case["num_surfaces"] * case["samples_per_ray"]
    return {k: torch.randn((n_cam, g) + tail, generator=gen, dtype=torch.float64) for k, tail in zip(OUTPUTS, ((), (), (2,)))}


def _run(fn, case, dtype, device, weights, use=OUTPUTS, xy_grad=True, backward_twice=False, forward_only=False):
    """outputs, index and gradients of one route, as float64 (index: int64) CPU tensors"""
    args = {k: (v.detach().clone().to(device=device, dtype=dtype) if torch.is_tensor(v) else v) for k, v in case.items()}
    if forward_only:
        out = _as_dict(fn(**args))
        return dict({k: out[k].detach().double().cpu() for k in OUTPUTS}, index=out["index"].detach().long().cpu())
    args["logits"].requires_grad_(True)
    args["xy_raw"].requires_grad_(xy_grad)
    out = _as_dict(fn(**args))
    loss = sum((out[k] * weights[k].to(device=device, dtype=dtype)).sum() for k in use)
    leaves = [args[k] for k in LEAVES if args[k].requires_grad]
    names = [k for k in LEAVES if args[k].requires_grad]
    grads = torch.autograd.grad(loss, leaves, retain_graph=backward_twice, allow_unused=True)
    res = {k: out[k].detach().double().cpu() for k in OUTPUTS}
    res["index"] = out["index"].detach().long().cpu()
    res.update({"d_" + k: g.double().cpu() for k, g in zip(names, grads) if g is not None})
    if backward_twice:
        res["second"] = {"d_" + k: g.double().cpu() for k, g in zip(names, torch.autograd.grad(loss, leaves))}
    return res


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def _three_routes(case, seed, **kw):
    from ggrt_official_amd import fused_depth_head
    w = _weights(case, seed)
    ref = _run(depth_head_reference, case, torch.float64, "cpu", w, **kw)
    t32 = _run(depth_head_reference, case, torch.float32, DEV, w, **kw)
    ker = _run(fused_depth_head, case, torch.float32, DEV, w, **kw)
    return ref, t32, ker


def _routes(n_cam, rays, s, srf, spp, mode, transmittance=False, exponent=1.0):
    seed = 7 * n_cam + rays + 13 * spp + 3 * s + srf
    case = make_case(n_cam, rays, s, srf, spp, mode, seed=seed, use_transmittance=transmittance, opacity_exponent=exponent)
    return (case,) + _three_routes(case, seed)


def _hold_to_the_bar(ref, t32, ker, what="", zero_ok=()):
    assert torch.equal(ker["index"], ref["index"]), (what, int((ker["index"] != ref["index"]).sum()))
    assert torch.equal(t32["index"], ref["index"]), what     # (the margin rule at work: the float32 torch route chooses alike)
    bad = []
    for k, r in ref.items():
        if k in ("index", "second"):
            continue
        if float(r.abs().max()) == 0 and k in zero_ok:
            assert float(ker[k].abs().max()) == 0, k
            continue
        assert float(r.abs().max()) > 0, k
        e_k, e_t = _err(ker[k], r), _err(t32[k], r)
        print(f"{what} {k:14s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad


E2, EH = 2 ** 0.5, 2 ** -1
CASES = ([(c, h, 32, 1, 3, "sampled", False, 1.0) for c in (1, 3) for h in (1, 63, 64, 65, 257)] +
         [(c, h, 32, 1, 3, "deterministic", True, E2) for c in (1, 3) for h in (1, 63, 64, 65, 257)] +
         [(3, 65, s, 1, 3, "sampled", t, e) for s, t, e in ((1, False, E2), (2, True, E2), (31, False, EH), (33, True, E2), (64, True, 1.0))] +
         [(3, 65, s, 1, min(s, 3), "deterministic", t, e) for s, t, e in ((1, True, 1.0), (2, False, E2), (31, True, E2), (33, False, 1.0),
                                                                        (64, False, EH))] +
         [(3, 33, 32, 2, 3, m, t, E2) for m, t in (("sampled", True), ("deterministic", False))] +        # R·srf = 66
         [(1, 32, 32, 2, 1, "sampled", False, EH), (3, 129, 31, 2, 1, "deterministic", True, 1.0),        # R·srf = 64, 258
          (3, 43, 5, 3, 2, "sampled", True, E2), (3, 43, 5, 3, 2, "deterministic", False, E2)] +           # tiles end inside a ray
         [(3, 65, 32, 1, 1, "sampled", True, 1.0), (3, 65, 32, 1, 2, "deterministic", False, EH), (3, 65, 32, 1, 5, "sampled", False, E2),
          (3, 65, 16, 1, 16, "deterministic", True, E2), (3, 65, 16, 1, 16, "sampled", False, EH)] +     # spp = s; every KMAX
         [(3, 44801, 2, 1, 1, "sampled", True, E2)])                                                       # beyond the maximum grid


@pytest.mark.parametrize("n_cam,rays,s,srf,spp,mode,transmittance,exponent", CASES)
def test_index_outputs_and_gradients_match_the_float64_restatement(n_cam, rays, s, srf, spp, mode, transmittance, exponent):
    _, ref, t32, ker = _routes(n_cam, rays, s, srf, spp, mode, transmittance, exponent)
    assert set(ref) == set(OUTPUTS) | {"index"} | {"d_" + k for k in LEAVES}
    assert int(ref["index"].min()) >= 0 and int(ref["index"].max()) < s
    _hold_to_the_bar(ref, t32, ker, f"C={n_cam} R={rays} s={s} srf={srf} spp={spp} {mode} T={transmittance} e={exponent:.3f}")


@pytest.mark.parametrize("n_cam,rays,s,spp,mode", [(3, 65, 2, 3, "sampled"), (3, 257, 32, 3, "sampled"), (3, 65, 32, 3, "deterministic"),
                                                  (3, 65, 5, 5, "deterministic")])
def test_the_forward_of_the_transmittance_form_with_an_exponent_below_one(n_cam, rays, s, spp, mode):
    """forward only (the module's docstring says why no gradients): where the last bucket is chosen q is 1 up to rounding, the
    reference's (1 − q)^e is NaN when it rounds above, and the kernel's base is max(1 − q, 0) — index, depths and opacities are
    held to the bar, and everything is finite"""
    from ggrt_official_amd import fused_depth_head
    seed = 17 + rays + s
    case = make_case(n_cam, rays, s, 1, spp, mode, seed=seed, use_transmittance=True, opacity_exponent=EH)
    w = _weights(case, seed)
    ref, t32, ker = (_run(fn, case, dt, dev, w, forward_only=True) for fn, dt, dev in
                     ((depth_head_reference, torch.float64, "cpu"), (depth_head_reference, torch.float32, DEV),
                      (fused_depth_head, torch.float32, DEV)))
    assert bool((ref["index"] == s - 1).any())     # (the clamp's place is visited)
    assert all(bool(torch.isfinite(ker[k]).all()) for k in OUTPUTS)
    _hold_to_the_bar(ref, t32, ker, f"forward, T=True e=0.5, s={s} {mode}")


@pytest.mark.parametrize("transmittance,exponent", [(False, E2), (True, E2), (False, 1.0)])
def test_a_peaked_pdf_puts_every_sample_into_one_bucket(transmittance, exponent):
    """the backward's repeated-index sum: three samples of a head in the same bucket"""
    case = make_case(3, 65, 32, 1, 3, "sampled", seed=5, use_transmittance=transmittance, opacity_exponent=exponent, logit_scale=0.5)
    peak = torch.arange(3 * 65).reshape(3, 65) % 32
    case["logits"][..., 0::2].scatter_add_(-1, peak[..., None], torch.full((3, 65, 1), 9.0, dtype=torch.float64))
    case["u"] = torch.tensor([0.3, 0.5, 0.7], dtype=torch.float64).expand(3, 65, 1, 3).contiguous()
    assert not bool(margin_violations(case["logits"], 1, 3, False, case["u"]).any())
    ref, t32, ker = _three_routes(case, 5)
    assert torch.equal(ref["index"].reshape(3, 65, 3), peak[..., None].expand(3, 65, 3))
    _hold_to_the_bar(ref, t32, ker, f"peaked T={transmittance}")


def test_u_just_below_one_is_clipped_to_the_last_bucket():
    case = make_case(3, 65, 32, 1, 3, "sampled", seed=6)
    case["u"] = torch.full_like(case["u"], 1.0 - 2.0 ** -24)
    ref, t32, ker = _three_routes(case, 6)
    assert bool((ref["index"] == 31).all())
    _hold_to_the_bar(ref, t32, ker, "u -> 1")


def test_a_strided_xy_raw_view_is_read_in_place_with_identical_bits():
    from ggrt_official_amd import fused_depth_head
    case = make_case(3, 65, 32, 2, 3, "sampled", seed=8, use_transmittance=True, opacity_exponent=E2)
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    w = {k: v.to(device=DEV, dtype=torch.float32) for k, v in _weights(case, 8).items()}
    wide = torch.randn(3, 130, 9, device=DEV)
    wide[..., :2] = args["xy_raw"]
    res = []
    for xy in (wide.clone().requires_grad_(True), args["xy_raw"].clone().requires_grad_(True)):
        logits = args["logits"].clone().requires_grad_(True)
        view = xy[..., :2] if xy.shape[-1] == 9 else xy
        out = _as_dict(fused_depth_head(**dict(args, logits=logits, xy_raw=view)))
        g_l, g_xy = torch.autograd.grad(sum((out[k] * w[k]).sum() for k in OUTPUTS), [logits, xy])
        res.append([out[k] for k in OUTPUTS + ("index",)] + [g_l, g_xy[..., :2]])
        assert xy.shape[-1] == 2 or float(g_xy[..., 2:].abs().max()) == 0
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_every_output_and_gradient_is_written_whole(monkeypatch):
    """the wrapper's buffers pre-filled with NaN (index: −1): none survives, at ragged tiles and with tiles that end inside a ray"""
    from ggrt_official_amd import splatting
    monkeypatch.setattr(splatting, "_DEPTH_HEAD_POISON", True)
    for mode in ("sampled", "deterministic"):
        case = make_case(3, 43, 5, 3, 2, mode, seed=9, use_transmittance=True, opacity_exponent=E2)
        ker = _run(splatting.fused_depth_head, case, torch.float32, DEV, _weights(case, 9))
        ref = _run(depth_head_reference, case, torch.float64, "cpu", _weights(case, 9))
        for k, v in ker.items():
            assert bool(torch.isfinite(v.double()).all()) and v.shape == ref[k].shape, k
        assert torch.equal(ker["index"], ref["index"])
        # and only the chosen buckets' offset logits carry a gradient
        d_off = ker["d_logits"].reshape(3, 43, 5, 3, 2)[..., 1].permute(0, 1, 3, 2)
        chosen = torch.zeros(3, 43, 3, 5).scatter_(-1, ref["index"].reshape(3, 43, 3, 2), 1.0).bool()
        assert float(d_off[~chosen].abs().max()) == 0 and float(d_off[chosen].abs().min()) > 0


def test_two_backward_runs_give_identical_bits():
    case = make_case(3, 257, 32, 1, 3, "sampled", seed=10, use_transmittance=True, opacity_exponent=E2)
    from ggrt_official_amd import fused_depth_head
    ker = _run(fused_depth_head, case, torch.float32, DEV, _weights(case, 10), backward_twice=True)
    for k, v in ker["second"].items():
        assert torch.equal(v, ker[k]), k


@pytest.mark.parametrize("use", [("opacities", "coordinates"), ("depths", "coordinates"), ("depths", "opacities"), ("coordinates",)])
def test_absent_output_gradients_are_taken_as_zero(use):
    case = make_case(3, 65, 32, 1, 3, "sampled", seed=11, use_transmittance=True, opacity_exponent=E2)
    ref, t32, ker = _three_routes(case, 11, use=use)
    zero = ("d_logits",) if use == ("coordinates",) else ()
    if zero:     # (torch reports an unused leaf as no gradient at all: the kernels write zeros)
        ref["d_logits"] = t32["d_logits"] = torch.zeros_like(ker["d_logits"])
    _hold_to_the_bar(ref, t32, ker, f"loss over {use}", zero_ok=zero)


def test_xy_raw_without_grad():
    case = make_case(3, 65, 32, 1, 3, "deterministic", seed=12)
    ref, t32, ker = _three_routes(case, 12, xy_grad=False)
    assert "d_xy_raw" not in ker and "d_logits" in ker
    _hold_to_the_bar(ref, t32, ker, "no xy_raw grad")


def test_no_cameras():
    from ggrt_official_amd import fused_depth_head
    case = make_case(1, 5, 32, 1, 3, "sampled", seed=13)
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    for k in ("logits", "xy_raw", "near", "far", "u"):
        args[k] = args[k][:0]
    args["logits"].requires_grad_(True)
    out = fused_depth_head(**args)
    assert out.depths.shape == (0, 15) and out.opacities.shape == (0, 15) and out.coordinates.shape == (0, 15, 2) and out.index.shape == (0, 15)
    (g,) = torch.autograd.grad(out.depths.sum() + out.opacities.sum(), [args["logits"]])
    assert g.shape == (0, 5, 64)


def test_u_none_draws_on_the_device_from_torchs_generator():
    from ggrt_official_amd import fused_depth_head
    case = make_case(3, 65, 32, 1, 3, "sampled", seed=14)
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    args["u"] = None
    state = torch.cuda.get_rng_state(DEV)
    first = fused_depth_head(**args)
    other = fused_depth_head(**args)
    torch.cuda.set_rng_state(state, DEV)
    again = fused_depth_head(**args)
    assert first.index.dtype == torch.int32 and int(first.index.min()) >= 0 and int(first.index.max()) < 32
    assert torch.equal(first.index, again.index) and torch.equal(first.depths, again.depths) and torch.equal(first.opacities, again.opacities)
    assert not torch.equal(first.index, other.index)


def test_invalid_shapes_are_refused():
    from ggrt_official_amd import fused_depth_head
    case = make_case(2, 12, 4, 1, 3, "sampled", seed=0)
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    with pytest.raises(ValueError):
        fused_depth_head(**dict(args, logits=args["logits"][..., :-1].contiguous()))
    with pytest.raises(ValueError):
        fused_depth_head(**dict(args, xy_raw=args["xy_raw"][:, :-1]))
    with pytest.raises(ValueError):
        fused_depth_head(**dict(args, u=args["u"][:, :-1]))
    with pytest.raises(ValueError):     # (the right number of elements in another order of axes)
        fused_depth_head(**dict(args, xy_raw=args["xy_raw"].reshape(2, 1, 12, 2)))
    assert fused_depth_head(**dict(args, xy_raw=args["xy_raw"].reshape(2, 12, 1, 2))).depths.shape == (2, 36)
    with pytest.raises(RuntimeError, match="samples_per_ray"):
        fused_depth_head(**dict(args, deterministic=True, samples_per_ray=5, u=None))
