"""What folding the depth encoding into the epipolar attention kernels buys beside the route without the fold, on one GPU.

GGRt's training shape: 2 context views × 120 × 88 rays, so N = 21 120 rays of S = 32 samples, C = 128 channels, H = 4 heads of
D = 128 (dim = 128), a positional encoding of O = 10 octaves, and TWO attention layers over one (features, depth) pair and one
`depth_encoding`, each  x = x + Attention(x, features + Linear(PE(depth)))  (the LayerNorm, which both routes would share, is left
out).  One step is a forward plus the backward from a fixed random upstream gradient to x, features, w_enc, b_enc and every
attention weight.
  route P   the parent's: the encoding in float32 torch (PE, Linear, add: z is built once and shared by the layers), then
            `fused_epipolar_attention` twice on z
  route E   `fused_epipolar_encoded_attention` twice on the raw features and depth (csrc/epipolar_attn_enc.hip): z is never built
The routes are warmed up, then timed ALTERNATELY with HIP events around each step, so that a drift of the machine hits both.  Each
route's `torch.cuda.max_memory_allocated` over a step, above what is allocated once the inputs exist, is recorded too.  The two
kernels are also timed on their own (events around `epipolar_encoded_attention_core`'s forward and around its backward, without
dL/ddepth, as in the step), against the bytes they must move: forward features + depth + qk + qe + ctx_f + ctx_e + attn, backward
the inputs, attn and both upstream gradients read, g_qk, g_qe and g_f written.  Prints one JSON line and, with --out, writes it.

    python scripts/epipolar_encoded_attention_cost.py --steps 20 --warmup 3 --out profiles/epipolar_encoded_attention_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import epipolar_encoded_attention_core, fused_epipolar_attention, fused_epipolar_encoded_attention  # noqa: E402
from tests.epipolar_encoded_attention_reference import positional_encoding  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12      # the MI355X's specified HBM3E rate


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(x):
    q = statistics.quantiles(x, n=4)
    return {"ms": [round(statistics.median(x), 4), round(min(x), 4), round(max(x), 4)], "iqr_ms": round(q[2] - q[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=2 * 120 * 88)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--dim-head", type=int, default=128)
    ap.add_argument("--octaves", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epipolar_encoded_attention_cost.py measures on the GPU: none found")
    n, s, c, h, d, o = a.rays, a.samples, a.channels, a.heads, a.dim_head, a.octaves
    dim, inner, e = c, h * d, 2 * o
    gen = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.randn(shape, generator=gen).to(DEV)
    x, features, g_out = r(n, 1, dim).requires_grad_(True), r(n, s, c).requires_grad_(True), r(n, 1, dim)
    depth = torch.rand((n, s), generator=gen).to(DEV)
    w_enc, b_enc = (r(c, e) / e ** 0.5).requires_grad_(True), r(c).requires_grad_(True)
    layers = [[(r(inner, dim) / dim ** 0.5).requires_grad_(True), (r(2 * inner, c) / c ** 0.5).requires_grad_(True),
               (r(dim, inner) / inner ** 0.5).requires_grad_(True), r(dim).requires_grad_(True)] for _ in range(2)]
    leaves = [x, features, w_enc, b_enc] + [w for layer in layers for w in layer]
    res = {"rays": n, "samples": s, "channels": c, "heads": h, "dim_head": d, "dim": dim, "octaves": o, "layers": 2, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "features_bytes": n * s * c * 4}

    def route_p():
        z = features + torch.nn.functional.linear(positional_encoding(depth, o), w_enc, b_enc)
        y = x
        for layer in layers:
            y = y + fused_epipolar_attention(y, z, *layer, h)
        return y

    def route_e():
        y = x
        for layer in layers:
            y = y + fused_epipolar_encoded_attention(y, features, depth, w_enc, b_enc, *layer, h)
        return y

    routes = {"P_encoding_in_torch": route_p, "E_encoding_in_kernel": route_e}

    def step(fn):
        y = fn()
        return (y.detach(),) + torch.autograd.grad(y, leaves, g_out)

    first = {name: step(fn) for name, fn in routes.items()}          # (also the first warm-up)
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
    p0, e0 = first["P_encoding_in_torch"], first["E_encoding_in_kernel"]
    agree = {"max_rel_difference_of_output": rel(e0[0], p0[0]), "max_rel_difference_of_dfeatures": rel(e0[2], p0[2]),
             "max_rel_difference_of_dw_enc": rel(e0[3], p0[3]), "max_rel_difference_of_db_enc": rel(e0[4], p0[4])}
    del first, p0, e0
    for _ in range(a.warmup):
        for fn in routes.values():
            step(fn)
    ms, peak = {name: [] for name in routes}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(fn)
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - before)
    for _ in range(a.steps):
        for name, fn in routes.items():
            ms[name].append(timed(lambda: step(fn))[0])
    stats = {name: summary(v) for name, v in ms.items()}
    med_p, med_e = stats["P_encoding_in_torch"]["ms"][0], stats["E_encoding_in_kernel"]["ms"][0]
    larger_iqr = max(st["iqr_ms"] for st in stats.values())
    res["step"] = {**{name: {**stats[name], "peak_bytes_above_inputs": peak[name]} for name in routes},
                   "P_over_E": round(med_p / med_e, 3), "median_P_minus_median_E_ms": round(med_p - med_e, 4), "larger_iqr_ms": larger_iqr,
                   "E_is_below_P_by_more_than_the_larger_iqr": bool(med_p - med_e > larger_iqr),
                   "peak_P_over_E": round(peak["P_encoding_in_torch"] / max(peak["E_encoding_in_kernel"], 1), 2), **agree}

    # the two kernels alone
    qk, qe = r(n, h, c).mul_(0.1).requires_grad_(True), r(n, h, e).mul_(0.1).requires_grad_(True)
    ff = features.detach().clone().requires_grad_(True)
    g_f, g_e = r(n, h, c), r(n, h, e)
    fwd_ms, bwd_ms = [], []
    for i in range(a.warmup + a.steps):
        t_f, (ctx_f, ctx_e, _) = timed(lambda: epipolar_encoded_attention_core(qk, qe, ff, depth))
        t_b, _ = timed(lambda: torch.autograd.grad([ctx_f, ctx_e], [qk, qe, ff], [g_f, g_e]))
        if i >= a.warmup:
            fwd_ms.append(t_f)
            bwd_ms.append(t_b)
    small = n * h * (c + e) * 4
    fwd_bytes = n * s * c * 4 + n * s * 4 + 2 * small + n * h * s * 4
    bwd_bytes = fwd_bytes + small + n * s * c * 4      # qk, qe, features, depth, attn, g_f_ctx, g_e_ctx read; g_qk, g_qe, g_f written
    for name, v, nbytes in (("kernel_forward", fwd_ms, fwd_bytes), ("kernel_backward", bwd_ms, bwd_bytes)):
        m = statistics.median(v)
        res[name] = {**summary(v), "bytes_to_move": int(nbytes), "GB_per_s": round(nbytes / m / 1e6, 1),
                     "share_of_hbm_rate": round(nbytes / (m * 1e-3) / HBM_BYTES_PER_S, 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
