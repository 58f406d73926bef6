"""`fused_epipolar_sampler` where GGRt's EpipolarTransformer.forward would call it: q = features + Linear(PE(depth)), the key/value
tensor of the epipolar attention, through the fused sampler and through the torch restatement (float64 on the CPU, float32 on
the device).  v = 2, 12 × 8 rays, s = 8, c = 16; PE is a 10-octave sin / cos positional encoding written here; the loss is
Σ q · fixed random weights.  q, dL/dimages and dL/dLinear.weight are held to  e_kernel <= max(4·e_torch32, 1e-6),
e = max|x − ref64| / max|ref64|."""
import math

import pytest
import torch
from torch import nn

from tests.epipolar_reference import epipolar_reference, make_case, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OCTAVES = 10


def positional_encoding(x):
    """[..., 1] -> [..., 2·OCTAVES]: sin and cos of 2π·2^k·x, k < OCTAVES"""
    freq = 2 * math.pi * 2.0 ** torch.arange(OCTAVES, dtype=x.dtype, device=x.device)
    phase = x * freq
    return torch.cat([phase.sin(), phase.cos()], dim=-1)


def _route(sampler, case, dtype, device, weights):
    torch.manual_seed(5)
    linear = nn.Linear(2 * OCTAVES, 16).to(device=device, dtype=dtype)
    images = case["images"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    out = run_case(sampler, dict(case, images=images), dtype, device)
    features, depth = (out["features"], out["depth"]) if isinstance(out, dict) else (out.features, out.depth)
    assert not depth.requires_grad
    q = features + linear(positional_encoding(depth[..., None]))
    loss = (q * weights.to(device=device, dtype=dtype)).sum()
    g_images, g_weight = torch.autograd.grad(loss, [images, linear.weight])
    return dict(q=q.detach().double().cpu(), d_images=g_images.double().cpu(), d_weight=g_weight.double().cpu())


def test_the_attention_input_and_its_gradients_match_the_restatement():
    from ggrt_official_amd import fused_epipolar_sampler
    case = make_case(1, 2, 12, 8, 16, 8, 31)
    weights = torch.randn((1, 2, 1, 96, 8, 16), generator=torch.Generator().manual_seed(32), dtype=torch.float64)
    ref = _route(epipolar_reference, case, torch.float64, "cpu", weights)
    t32 = _route(epipolar_reference, case, torch.float32, DEV, weights)
    ker = _route(fused_epipolar_sampler, case, torch.float32, DEV, weights)
    err = lambda x, r: float((x - r).abs().max() / r.abs().max())
    bad = []
    for k, r in ref.items():
        e_k, e_t = err(ker[k], r), err(t32[k], r)
        print(f"{k:9s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad


def test_a_camera_tensor_that_requires_grad_raises():
    from ggrt_official_amd import fused_epipolar_sampler
    case = make_case(1, 2, 12, 8, 16, 8, 31)
    args = {k: case[k].to(device=DEV, dtype=torch.float32) for k in ("images", "extrinsics", "intrinsics", "near", "far")}
    with pytest.raises(RuntimeError, match="camera gradients are not implemented"):
        fused_epipolar_sampler(**dict(args, extrinsics=args["extrinsics"].clone().requires_grad_(True)), num_samples=8)
    out = fused_epipolar_sampler(**dict(args, extrinsics=args["extrinsics"].clone().requires_grad_(True).detach()), num_samples=8)
    assert out.features.shape == (1, 2, 1, 96, 8, 16) and out.valid.dtype == torch.bool
