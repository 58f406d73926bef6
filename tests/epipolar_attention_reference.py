"""GGRt's epipolar cross-attention (`Attention.forward(x, z)` of transformer/attention.py as `EpipolarTransformer.forward` calls it: ONE
query token per ray, the ray's S samples as keys and values, z not normed) restated in torch from its formulas, in any dtype and on
any device:

* `attention_literal`: K and V materialised over all N·S sample tokens, as the reference runs it;
* `attention_folded`: the key projection folded into the query and the value projection applied after the weighted sum — the
  route of `fused_epipolar_attention`, with `core_forward` where the HIP kernel stands;
* `core_forward` / `core_backward`: the per-ray core and the four backward formulas of include/ggr_raster.h
  (GgrEpipolarAttnPass), the latter written out by hand so that gradcheck can hold them against autograd.

Weights are the reference's `nn.Linear` weights: w_q [H·D, dim], w_kv [2·H·D, kv_dim] (K rows first, head-major), w_out [dim, H·D]
and b_out [dim], or None / None when the reference has no output projection (H = 1 and D = dim)."""
import torch

WEIGHTS = ("w_q", "w_kv", "w_out", "b_out")


def attention_literal(x, z, w_q, w_kv, w_out, b_out, heads):
    """x [N,1,dim] (or [N,dim]), z [N,S,kv_dim] -> x's shape"""
    n, s = z.shape[0], z.shape[1]
    inner = w_q.shape[0]
    d = inner // heads
    q = (x.reshape(n, 1, -1) @ w_q.t()).reshape(n, 1, heads, d).permute(0, 2, 1, 3)            # [N,H,1,D]
    kv = z @ w_kv.t()                                                                           # [N,S,2·H·D]
    k = kv[..., :inner].reshape(n, s, heads, d).permute(0, 2, 1, 3)                             # [N,H,S,D]
    v = kv[..., inner:].reshape(n, s, heads, d).permute(0, 2, 1, 3)
    dots = (q @ k.transpose(-1, -2)) * d ** -0.5                                                # [N,H,1,S]
    attn = torch.softmax(dots, dim=-1)
    out = (attn @ v).permute(0, 2, 1, 3).reshape(n, 1, inner)
    if w_out is not None:
        out = out @ w_out.t() + b_out
    return out.reshape(x.shape)


def core_forward(qk, z):
    """qk [N,H,C], z [N,S,C] -> ctx [N,H,C], attn [N,H,S]"""
    logit = torch.einsum("nhc,nsc->nhs", qk, z)
    attn = torch.softmax(logit, dim=-1)
    return torch.einsum("nhs,nsc->nhc", attn, z), attn


def core_backward(qk, z, attn, g_ctx):
    """the four formulas of the backward pass -> g_qk [N,H,C], g_z [N,S,C]"""
    da = torch.einsum("nhc,nsc->nhs", g_ctx, z)
    dl = attn * (da - (attn * da).sum(-1, keepdim=True))
    g_qk = torch.einsum("nhs,nsc->nhc", dl, z)
    g_z = torch.einsum("nhs,nhc->nsc", attn, g_ctx) + torch.einsum("nhs,nhc->nsc", dl, qk)
    return g_qk, g_z


def attention_folded(x, z, w_q, w_kv, w_out, b_out, heads, core=core_forward):
    n = z.shape[0]
    inner, kv_dim = w_q.shape[0], z.shape[2]
    d = inner // heads
    q = (x.reshape(n, -1) @ w_q.t()).reshape(n, heads, d)
    wk, wv = w_kv[:inner].reshape(heads, d, kv_dim), w_kv[inner:].reshape(heads, d, kv_dim)
    qk = d ** -0.5 * torch.einsum("nhd,hdc->nhc", q, wk)
    ctx, _ = core(qk, z)
    out = torch.einsum("nhc,hdc->nhd", ctx, wv).reshape(n, inner)
    if w_out is not None:
        out = out @ w_out.t() + b_out
    return out.reshape(x.shape)


def make_case(n, s, dim, kv_dim, heads, d, seed, project_out=True, q_gain=1.0):
    """seeded float64 CPU inputs, weights and the upstream gradient; `q_gain` scales w_q (large logits)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    inner = heads * d
    case = dict(x=r(n, 1, dim), z=r(n, s, kv_dim), w_q=r(inner, dim) * (q_gain / dim ** 0.5), w_kv=r(2 * inner, kv_dim) / kv_dim ** 0.5,
                w_out=r(dim, inner) / inner ** 0.5 if project_out else None, b_out=r(dim) if project_out else None,
                g_out=r(n, 1, dim), heads=heads, seed=seed)
    assert project_out or (heads == 1 and d == dim)
    return case


def run_route(fn, case, dtype, device):
    """the output of `fn(x, z, w_q, w_kv, w_out, b_out, heads)` and every gradient for the case's upstream gradient, as float64 CPU
    tensors: {"out", "x", "z", "w_q", "w_kv"[, "w_out", "b_out"]}"""
    names = [k for k in ("x", "z") + WEIGHTS if case[k] is not None]
    leaf = {k: case[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    args = [leaf.get(k) for k in ("x", "z") + WEIGHTS]
    out = fn(*args, case["heads"])
    grads = torch.autograd.grad(out, [leaf[k] for k in names], case["g_out"].to(device=device, dtype=dtype).reshape(out.shape))
    res = {k: g.detach().double().cpu() for k, g in zip(names, grads)}
    res["out"] = out.detach().double().cpu()
    return res
