"""What the fused epipolar cross-attention costs beside the torch route it replaces, on one GPU.

GGRt's training shape: 2 context views × 120 × 88 rays, so N = 21 120 rays of S = 32 samples, C = 128 channels, H = 4 heads of
D = 128 (dim = 128): z is 86.5 M floats.  One step is a forward plus the backward from a fixed random upstream gradient to x, z
and every weight, for ONE attention layer and for TWO layers sharing z (each  x = x + Attention(x, z);  the LayerNorm, which
both routes would share, is left out).  The two routes — `fused_epipolar_attention` (csrc/epipolar_attn.hip between [N,·]-sized
torch GEMMs) and the literal float32 torch route (tests/epipolar_attention_reference.py `attention_literal`: `to_kv` over all
N·S sample tokens, as the reference runs it) — are warmed up, then timed ALTERNATELY with HIP events around each step, so that
a drift of the machine hits both.  Each route's `torch.cuda.max_memory_allocated` over a step, above what is allocated once
the inputs exist, is recorded too.  The two kernels are also timed on their own (events around `epipolar_attention_core`'s
forward and around its backward), against the bytes they must move: forward z + qk + ctx + attn, backward that plus g_ctx, g_qk
and g_z.  Prints one JSON line and, with --out, writes it to a file.

    python scripts/epipolar_attention_cost.py --steps 20 --warmup 3 --out profiles/epipolar_attention_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import epipolar_attention_core, fused_epipolar_attention  # noqa: E402
from tests.epipolar_attention_reference import attention_literal  # noqa: E402

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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epipolar_attention_cost.py measures on the GPU: none found")
    n, s, c, h, d = a.rays, a.samples, a.channels, a.heads, a.dim_head
    dim, inner = c, h * d
    gen = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.randn(shape, generator=gen).to(DEV)
    x, z, g_out = r(n, 1, dim).requires_grad_(True), r(n, s, c).requires_grad_(True), r(n, 1, dim)
    layers = [[(r(inner, dim) / dim ** 0.5).requires_grad_(True), (r(2 * inner, c) / c ** 0.5).requires_grad_(True),
               (r(dim, inner) / inner ** 0.5).requires_grad_(True), r(dim).requires_grad_(True)] for _ in range(2)]
    res = {"rays": n, "samples": s, "channels": c, "heads": h, "dim_head": d, "dim": dim, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "z_bytes": n * s * c * 4,
           "kv_bytes_per_layer_of_the_literal_route": n * s * 2 * inner * 4}
    routes = {"fused": fused_epipolar_attention, "torch32": attention_literal}

    for count in (1, 2):
        leaves = [x, z] + [w for layer in layers[:count] for w in layer]

        def step(fn):
            y = x
            for layer in layers[:count]:
                y = y + fn(y, z, *layer, h)
            return (y.detach(),) + torch.autograd.grad(y, leaves, g_out)

        first = {name: step(fn) for name, fn in routes.items()}          # (also the first warm-up)
        rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
        agree = {"max_rel_difference_of_output": rel(first["fused"][0], first["torch32"][0]),
                 "max_rel_difference_of_dz": rel(first["fused"][2], first["torch32"][2]),
                 "max_rel_difference_of_dw_kv": rel(first["fused"][4], first["torch32"][4])}
        del first
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
        med = {name: statistics.median(v) for name, v in ms.items()}
        res[f"layers_{count}"] = {**{name: {**summary(v), "peak_bytes_above_inputs": peak[name]} for name, v in ms.items()},
                                  "torch32_over_fused": round(med["torch32"] / med["fused"], 2),
                                  "peak_torch32_over_fused": round(peak["torch32"] / max(peak["fused"], 1), 2), **agree}

    # the two kernels alone
    qk = r(n, h, c).mul_(0.1).requires_grad_(True)
    zz = z.detach().clone().requires_grad_(True)
    g_ctx = r(n, h, c)
    fwd_ms, bwd_ms = [], []
    for i in range(a.warmup + a.steps):
        t_f, (ctx, _) = timed(lambda: epipolar_attention_core(qk, zz))
        t_b, _ = timed(lambda: torch.autograd.grad(ctx, [qk, zz], g_ctx))
        if i >= a.warmup:
            fwd_ms.append(t_f)
            bwd_ms.append(t_b)
    small = n * h * c * 4
    fwd_bytes = n * s * c * 4 + 2 * small + n * h * s * 4
    bwd_bytes = fwd_bytes + small + n * s * c * 4      # qk, z, attn, g_ctx read; g_qk, g_z written
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
