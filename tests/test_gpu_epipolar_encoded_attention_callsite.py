"""`fused_epipolar_encoded_attention` where GGRt's EpipolarTransformer.forward would call it, on the outputs of
`fused_epipolar_sampler` themselves: the sampler's `features` and `depth`, reshaped, go into both attention layers, each as
x = x + Attention(LayerNorm(x), features + Linear(PE(depth)))  with one shared `depth_encoding` (the reference's PreNorm norms x
only; its ConvFeedForward and ImageSelfAttention are not part of this).  One chain runs the fused sampler and the fused encoded
attention — z is never built; the other two run the torch restatements (tests/epipolar_reference.py, then the encoding in torch
and `attention_literal`) in float64 on the CPU and in float32 on the device, from the same inputs.  v = 2, 8 × 6 rays, s = 8,
c = 12, H = 2, D = 4, 10 octaves; the upstream gradient is fixed and random.  The output and the gradients with respect to the
feature maps, w_enc, b_enc and every other weight are held to  e_kernel <= max(4·e_torch32, 1e-6),  e = max|x − ref64| / max|ref64|."""
import pytest
import torch
import torch.nn.functional as F

from tests.epipolar_attention_reference import attention_literal
from tests.epipolar_encoded_attention_reference import positional_encoding
from tests.epipolar_reference import epipolar_reference, make_case, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OCTAVES = 10
C, S, HEADS, D, LAYERS = 12, 8, 2, 4, 2


def _weights():
    gen = torch.Generator().manual_seed(71)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    w = {"w_enc": r(C, 2 * OCTAVES) / (2 * OCTAVES) ** 0.5, "b_enc": r(C) * 0.1}
    for i in range(LAYERS):
        w.update({f"ln_w{i}": 1 + 0.1 * r(C), f"ln_b{i}": 0.1 * r(C), f"w_q{i}": r(HEADS * D, C) / C ** 0.5,
                  f"w_kv{i}": r(2 * HEADS * D, C) / C ** 0.5, f"w_out{i}": r(C, HEADS * D) / (HEADS * D) ** 0.5, f"b_out{i}": 0.1 * r(C)})
    return w


def _literal(x, features, depth, w_enc, b_enc, *rest):
    return attention_literal(x, features + F.linear(positional_encoding(depth, OCTAVES), w_enc, b_enc), *rest)


def _route(sampler, attention, case, weights, g_out, dtype, device):
    w = {k: t.detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k, t in weights.items()}
    images = case["images"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    out = run_case(sampler, dict(case, images=images), dtype, device)
    features, depth = (out["features"], out["depth"]) if isinstance(out, dict) else (out.features, out.depth)
    b, v, _, r = features.shape[:4]
    features, depth = features.reshape(b * v * r, S, C), depth.reshape(b * v * r, S)
    x = images.permute(0, 1, 3, 4, 2).reshape(b * v * r, 1, C)
    for i in range(LAYERS):      # both layers read the same pair
        normed = F.layer_norm(x, (C,), w[f"ln_w{i}"], w[f"ln_b{i}"])
        x = x + attention(normed, features, depth, w["w_enc"], w["b_enc"], w[f"w_q{i}"], w[f"w_kv{i}"], w[f"w_out{i}"], w[f"b_out{i}"], HEADS)
    names = ["images"] + list(w)
    grads = torch.autograd.grad(x, [images] + list(w.values()), g_out.to(device=device, dtype=dtype))
    res = {"d_" + k: g.double().cpu() for k, g in zip(names, grads)}
    res["out"] = x.detach().double().cpu()
    return res


def test_two_layers_on_the_samplers_own_features_and_depth_match_the_restatement_chain():
    from ggrt_official_amd import fused_epipolar_encoded_attention, fused_epipolar_sampler
    case = make_case(1, 2, 6, 8, C, S, 72)
    weights = _weights()
    g_out = torch.randn((2 * 48, 1, C), generator=torch.Generator().manual_seed(73), dtype=torch.float64)
    ref = _route(epipolar_reference, _literal, case, weights, g_out, torch.float64, "cpu")
    t32 = _route(epipolar_reference, _literal, case, weights, g_out, torch.float32, DEV)
    ker = _route(fused_epipolar_sampler, fused_epipolar_encoded_attention, case, weights, g_out, torch.float32, DEV)
    err = lambda x, r: float((x - r).abs().max() / r.abs().max())
    assert set(ker) == set(ref) and len(ref) == 2 + 2 + 6 * LAYERS
    bad = []
    for k, r in ref.items():
        assert ker[k].shape == r.shape and bool(torch.isfinite(ker[k]).all()), k
        e_k, e_t = err(ker[k], r), err(t32[k], r)
        print(f"{k:10s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad
