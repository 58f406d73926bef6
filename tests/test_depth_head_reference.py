"""tests/depth_head_reference.py (the restatement tests/test_gpu_depth_head.py holds the depth-head kernels to) against the
reference's own DepthPredictorMonocular.forward and EncoderEpipolar.map_pdf_to_opacity, recorded in tests/golden/depth_head_*.npz
(make_depth_head_golden.py), and its gradients against finite differences: no GPU.

The golden holds each case twice on the same projection output and uniform numbers: the reference in float32 and in float64.
Indices must match exactly (the golden's inputs obey the margin rule).  In float64 the restatement must reproduce the float64
golden to 1e-12; in float32 its error against the float64 golden may be at most 4 × the reference's own float32 error (its
float32 run against its float64 run), or 1e-6: float32 round-off, in another order of operations."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.depth_head_reference import depth_head_reference, make_case, margin_violations

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_head_*.npz")))


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def _restate(g, dtype, exponent=1.0):
    logits = torch.from_numpy(g["logits"])
    b, v, r, width = logits.shape
    srf, spp = int(g["num_surfaces"]), int(g["samples"])
    c = b * v
    out = depth_head_reference(
        logits.reshape(c, r, width).to(dtype), torch.zeros(c, r * srf, 2, dtype=dtype), torch.zeros(r, 2, dtype=dtype),
        torch.from_numpy(g["near"]).reshape(c).to(dtype), torch.from_numpy(g["far"]).reshape(c).to(dtype), (4, 4), srf, spp,
        bool(g["deterministic"]), use_transmittance=bool(g["use_transmittance"]), opacity_exponent=exponent, opacity_scale=1.0,
        u=torch.from_numpy(g["u"]).reshape(c, r, srf, spp).to(dtype) if "u" in g.files else None)
    return {k: t.reshape(b, v, r, srf, spp, *t.shape[2:]) for k, t in out.items()}


def test_the_golden_files_are_there():
    assert [os.path.basename(p) for p in GOLDEN] == ["depth_head_deterministic.npz", "depth_head_deterministic_transmittance.npz",
                                                     "depth_head_sampled.npz", "depth_head_sampled_transmittance.npz"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[11:-4] for p in GOLDEN])
def test_restatement_reproduces_the_reference(path):
    g = np.load(path, allow_pickle=False)
    logits = torch.from_numpy(g["logits"])
    u = torch.from_numpy(g["u"]).reshape(-1, logits.shape[2], int(g["num_surfaces"]), int(g["samples"])) if "u" in g.files else None
    assert not bool(margin_violations(logits.reshape(-1, *logits.shape[2:]), int(g["num_surfaces"]), int(g["samples"]),
                                      bool(g["deterministic"]), u).any())
    want_index = torch.from_numpy(g["index"])
    r64, r32 = _restate(g, torch.float64), _restate(g, torch.float32)
    assert torch.equal(r64["index"], want_index) and torch.equal(r32["index"], want_index)
    for ours, name in (("depths", "depth"), ("opacities", "opacity")):
        gold64, gold32 = torch.from_numpy(g[name + "64"]), torch.from_numpy(g[name + "32"]).double()
        assert _err(r64[ours], gold64) < 1e-12, name
        e_ours, e_ref = _err(r32[ours].double(), gold64), _err(gold32, gold64)
        print(f"{name}: restatement32 {e_ours:.3e}  reference32 {e_ref:.3e}")
        assert e_ours <= max(4 * e_ref, 1e-6), (name, e_ours, e_ref)
    # map_pdf_to_opacity at the stand-in cfg's exponents (1, 2**0.5, 2**-1)
    for i, (initial, final, warm_up, step) in enumerate(g["mapping_cfg"]):
        exponent = 2.0 ** (initial + min(step / warm_up, 1) * (final - initial))
        assert (i == 0) == (exponent == 1.0)
        gold64, gold32 = torch.from_numpy(g[f"mapped64_{i}"]), torch.from_numpy(g[f"mapped32_{i}"]).double()
        assert _err(_restate(g, torch.float64, exponent)["opacities"], gold64) < 1e-12, i
        # the reference's float32 run is NaN where the transmittance form rounds q above 1 ((1 − q)^e of a negative base): the
        # restatement clamps the base at 0 — the one stated deviation — and stays finite there; the reference's own error is
        # taken over its finite elements
        ok = torch.isfinite(gold32)
        assert bool(ok.all()) or bool(g["use_transmittance"])
        ours32 = _restate(g, torch.float32, exponent)["opacities"].double()
        assert bool(torch.isfinite(ours32).all())
        e_ours, e_ref = _err(ours32, gold64), float((gold32 - gold64)[ok].abs().max() / gold64.abs().max())
        print(f"mapped, exponent {exponent:.4f}: restatement32 {e_ours:.3e}  reference32 {e_ref:.3e}")
        assert e_ours <= max(4 * e_ref, 1e-6), (i, e_ours, e_ref)


@pytest.mark.parametrize("mode", ["sampled", "deterministic"])
@pytest.mark.parametrize("transmittance,exponent", [(False, 1.0), (True, 2 ** 0.5), (False, 2 ** -1)])
def test_gradients_match_finite_differences(mode, transmittance, exponent):
    case = make_case(2, 5, 4, 2, 3, mode, seed=3, use_transmittance=transmittance, opacity_exponent=exponent)
    index = depth_head_reference(**case)["index"]

    def fn(logits, xy_raw):
        out = depth_head_reference(**dict(case, logits=logits, xy_raw=xy_raw), index=index)
        return out["depths"], out["opacities"], out["coordinates"]

    assert torch.autograd.gradcheck(fn, (case["logits"].clone().requires_grad_(True), case["xy_raw"].clone().requires_grad_(True)))


def test_the_layout_and_the_coordinates():
    case = make_case(2, 6, 4, 2, 3, "sampled", seed=4, image_shape=(10, 20))
    out = depth_head_reference(**case)
    assert out["depths"].shape == (2, 36) and out["coordinates"].shape == (2, 36, 2) and out["index"].dtype == torch.int64
    coords = out["coordinates"].reshape(2, 6, 2, 3, 2)
    assert torch.equal(coords[..., 0, :], coords[..., 1, :]) and torch.equal(coords[..., 0, :], coords[..., 2, :])
    want = case["ray_xy"][None, :, None] + (torch.sigmoid(case["xy_raw"].reshape(2, 6, 2, 2)) - 0.5) * torch.tensor([1 / 20, 1 / 10], dtype=torch.float64)
    assert torch.allclose(coords[..., 0, :], want, rtol=1e-13, atol=1e-13)
    near, far = case["near"][:, None], case["far"][:, None]
    assert bool((out["depths"] > near * (1 - 1e-6)).all()) and bool((out["depths"] < far * (1 + 1e-6)).all())
    # the pdf logit of (ray, surface j, bucket d) is channel (d·srf + j)·2: moving one surface's logits moves only its heads
    moved = case["logits"].clone()
    moved.reshape(2, 6, 4, 2, 2)[:, :, :, 1, :] += 0.37
    other = depth_head_reference(**dict(case, logits=moved), index=out["index"])
    a, b = out["depths"].reshape(2, 6, 2, 3), other["depths"].reshape(2, 6, 2, 3)
    assert torch.equal(a[:, :, 0], b[:, :, 0]) and not torch.equal(a[:, :, 1], b[:, :, 1])
