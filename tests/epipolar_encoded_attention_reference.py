"""GGRt's epipolar cross-attention WITH its depth encoding (`EpipolarTransformer.forward` lines 120-121 and 157-160: the keys and
values are z = features + Linear(PositionalEncoding(depth[..., None])), then `Attention.forward(x, z)` with one query token per
ray) restated in torch from its formulas, in any dtype and on any device:

* `positional_encoding`: the reference's module on its own float32 constants F = float32(2π) and P = float32(π/2), evaluated in
  the dtype of `d` — in float64 that is the contract of GgrEpipolarAttnEncPass (include/ggr_raster.h);
* `encoded_literal`: the encoding, the Linear, the add, then `attention_literal` over the materialised z, as the reference runs it;
* `encoded_folded`: the route of `fused_epipolar_encoded_attention`, with `enc_core_forward` where the HIP kernel stands;
* `enc_core_forward` / `enc_core_backward`: the per-ray core and its backward formulas, the latter written out by hand so that
  gradcheck can hold them against autograd.

`w_enc` [C, 2·O] and `b_enc` [C] are the weight and bias of the encoding's `nn.Linear`; the other weights as in
tests/epipolar_attention_reference.py."""
import numpy as np
import torch

from tests.epipolar_attention_reference import WEIGHTS, attention_literal, make_case

F = float(np.float32(2 * np.pi))      # 6.2831854820251465, bits 0x40C90FDB
P = float(np.float32(np.pi / 2))      # 1.5707963705062866, bits 0x3FC90FDB
ENC_WEIGHTS = ("w_enc", "b_enc")
ENC_LEAVES = ("x", "features", "depth") + ENC_WEIGHTS + WEIGHTS


def positional_encoding(d, num_octaves):
    """d [...] -> [..., 2·O]: pe[2k+p] = sin(F·2^k·d + p·P)"""
    freq = F * 2.0 ** torch.arange(num_octaves, dtype=d.dtype, device=d.device)
    phase = torch.tensor([0.0, P], dtype=d.dtype, device=d.device)
    return torch.sin(d[..., None, None] * freq[:, None] + phase).reshape(*d.shape, 2 * num_octaves)


def encoding_derivative(d, num_octaves):
    """d pe / d d: F·2^k·cos(F·2^k·d + p·P)"""
    freq = F * 2.0 ** torch.arange(num_octaves, dtype=d.dtype, device=d.device)
    phase = torch.tensor([0.0, P], dtype=d.dtype, device=d.device)
    return (freq[:, None] * torch.cos(d[..., None, None] * freq[:, None] + phase)).reshape(*d.shape, 2 * num_octaves)


def encoded_literal(x, features, depth, w_enc, b_enc, w_q, w_kv, w_out, b_out, heads):
    pe = positional_encoding(depth, w_enc.shape[1] // 2)
    z = features + torch.nn.functional.linear(pe, w_enc, b_enc)
    return attention_literal(x, z, w_q, w_kv, w_out, b_out, heads)


def enc_core_forward(qk, qe, f, d):
    """qk [N,H,C], qe [N,H,E], f [N,S,C], d [N,S] -> ctx_f [N,H,C], ctx_e [N,H,E], attn [N,H,S]"""
    pe = positional_encoding(d, qe.shape[-1] // 2)
    logit = torch.einsum("nhc,nsc->nhs", qk, f) + torch.einsum("nhe,nse->nhs", qe, pe)
    attn = torch.softmax(logit, dim=-1)
    return torch.einsum("nhs,nsc->nhc", attn, f), torch.einsum("nhs,nse->nhe", attn, pe), attn


def enc_core_backward(qk, qe, f, d, attn, g_f_ctx, g_e_ctx):
    """the backward formulas of GgrEpipolarAttnEncPass -> g_qk [N,H,C], g_qe [N,H,E], g_f [N,S,C], g_d [N,S]"""
    o = qe.shape[-1] // 2
    pe = positional_encoding(d, o)
    da = torch.einsum("nhc,nsc->nhs", g_f_ctx, f) + torch.einsum("nhe,nse->nhs", g_e_ctx, pe)
    dl = attn * (da - (attn * da).sum(-1, keepdim=True))
    g_qk = torch.einsum("nhs,nsc->nhc", dl, f)
    g_qe = torch.einsum("nhs,nse->nhe", dl, pe)
    g_f = torch.einsum("nhs,nhc->nsc", attn, g_f_ctx) + torch.einsum("nhs,nhc->nsc", dl, qk)
    g_pe = torch.einsum("nhs,nhe->nse", attn, g_e_ctx) + torch.einsum("nhs,nhe->nse", dl, qe)
    return g_qk, g_qe, g_f, (g_pe * encoding_derivative(d, o)).sum(-1)


def encoded_folded(x, features, depth, w_enc, b_enc, w_q, w_kv, w_out, b_out, heads, core=enc_core_forward):
    n = features.shape[0]
    inner, kv_dim = w_q.shape[0], features.shape[2]
    dh = inner // heads
    q = (x.reshape(n, -1) @ w_q.t()).reshape(n, heads, dh)
    wk, wv = w_kv[:inner].reshape(heads, dh, kv_dim), w_kv[inner:].reshape(heads, dh, kv_dim)
    qk = dh ** -0.5 * torch.einsum("nhd,hdc->nhc", q, wk)
    ctx_f, ctx_e, _ = core(qk, qk @ w_enc, features, depth)
    out = torch.einsum("nhc,hdc->nhd", ctx_f, wv) + torch.einsum("nhe,hde->nhd", ctx_e, wv @ w_enc)
    if b_enc is not None:
        out = out + wv @ b_enc
    out = out.reshape(n, inner)
    if w_out is not None:
        out = out @ w_out.t() + b_out
    return out.reshape(x.shape)


def make_enc_case(n, s, dim, kv_dim, heads, d, num_octaves, seed, project_out=True, q_gain=1.0):
    """`make_case` (its z is the features) plus depth uniform in [0, 1] and the encoding's Linear, from a generator of their own.
    The depths are float32 numbers (held as float64): a float32 route then reads the very depths the float64 route reads — at
    octave k a rounding of d by 3e-8 would alone move the phase by 2e-7·2^k, in every float32 route alike."""
    case = make_case(n, s, dim, kv_dim, heads, d, seed, project_out, q_gain)
    gen = torch.Generator().manual_seed(seed + 1_000_003)
    e = 2 * num_octaves
    case["features"] = case.pop("z")
    case["depth"] = torch.rand((n, s), generator=gen, dtype=torch.float32).double()
    case["w_enc"] = torch.randn((kv_dim, e), generator=gen, dtype=torch.float64) / e ** 0.5
    case["b_enc"] = torch.randn((kv_dim,), generator=gen, dtype=torch.float64)
    case["num_octaves"] = num_octaves
    return case


def run_enc_route(fn, case, dtype, device):
    """the output of `fn(x, features, depth, w_enc, b_enc, w_q, w_kv, w_out, b_out, heads)` and every gradient for the case's
    upstream gradient, as float64 CPU tensors keyed "out" and by ENC_LEAVES"""
    names = [k for k in ENC_LEAVES if case[k] is not None]
    leaf = {k: case[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    out = fn(*[leaf.get(k) for k in ENC_LEAVES], case["heads"])
    grads = torch.autograd.grad(out, [leaf[k] for k in names], case["g_out"].to(device=device, dtype=dtype).reshape(out.shape))
    res = {k: g.detach().double().cpu() for k, g in zip(names, grads)}
    res["out"] = out.detach().double().cpu()
    return res
