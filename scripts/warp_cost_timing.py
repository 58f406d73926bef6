"""What the fused feature-metric cost map costs beside the torch route it replaces, on one GPU.

GGRt's shape: C = 128 feature channels at 48 x 63 (378 x 504 at 1/8) with V = 5 reference views (pretraining) and V = 7
(finetuning), in both forms: "mean" is one `depth_cost_calc` (a depth-GRU step), "none" the V `get_cost_each` of one pose-GRU step.
One step is the forward plus the backward to both feature maps, the inverse depth and the poses.  The two routes —
`fused_warp_cost` (csrc/warp_cost.hip) and a float32 torch route on the same device — are warmed up, then timed ALTERNATELY with HIP
events around each step, so that a drift of the machine hits both.  The torch route is the restatement's geometry
(tests/warp_cost_reference.py: `projected`) followed by `F.grid_sample`, as the reference samples; it is kinder to torch than the
reference is: no `Camera` objects, no 4 x 4 `.inverse()`, no `.to(device)`.  Each route's `torch.cuda.max_memory_allocated` over a
step, above what is allocated once the inputs exist, is recorded too.  Prints one JSON line and, with --out, writes it to a file.

    python scripts/warp_cost_timing.py --steps 30 --warmup 5 --out profiles/warp_cost_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_warp_cost  # noqa: E402
from tests.warp_cost_reference import INPUTS, make_warp_case, projected  # noqa: E402

DEV = "cuda:0"
C, H, W, SCALE = 128, 48, 63, 1.0 / 8


def torch_route(fmap, fmaps_ref, inv_depth, K, ref_Ks, poses, reduce):
    costs = []
    for j in range(fmaps_ref.shape[0]):
        P = projected(inv_depth, K, ref_Ks[j], poses[j], SCALE)
        Z = P[2].clamp(min=1e-5)
        grid = torch.stack([2 * (P[0] / Z) / (W - 1) - 1.0, 2 * (P[1] / Z) / (H - 1) - 1.0], -1)[None]
        costs.append((fmap - F.grid_sample(fmaps_ref[j:j + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True)) ** 2)
    return torch.stack(costs, 1).mean(1) if reduce == "mean" else torch.cat(costs, 0)


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


def compare(routes, step, steps, warmup):
    for _ in range(warmup + 1):
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
    for _ in range(steps):
        for name, fn in routes.items():
            ms[name].append(timed(lambda: step(fn))[0])
    out = {name: {**summary(v), "peak_bytes_above_inputs": peak[name]} for name, v in ms.items()}
    out["torch32_over_fused"] = round(out["torch32"]["ms"][0] / out["fused"]["ms"][0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_cost_timing.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for V in (5, 7):
        case = {k: v.to(device=DEV, dtype=torch.float32).contiguous() for k, v in make_warp_case(V, C, H, W, 60 + V, scale_factor=SCALE).items()}
        leaves = [case[k].requires_grad_(True) for k in INPUTS]
        for form in ("mean", "none"):
            routes = {"fused": lambda *x: fused_warp_cost(*x, scale_factor=SCALE, reduce=form),
                      "torch32": lambda f, r, d, K, Ks, p: torch_route(f, r, d, K, Ks, p, form)}

            def step(fn):
                cost = fn(case["fmap"], case["fmaps_ref"], case["inv_depth"], case["K"], case["ref_Ks"], case["poses"])
                return (cost,) + torch.autograd.grad((cost * case["g_" + form]).sum(), leaves)

            first = {name: step(fn) for name, fn in routes.items()}
            entry = compare(routes, step, a.steps, a.warmup)
            entry["max_rel_difference"] = {k: float((x - y).abs().max() / y.abs().max()) for k, x, y in zip(("cost",) + INPUTS, first["fused"], first["torch32"])}
            fwd, bwd = [], []
            for i in range(a.warmup + a.steps):
                t_f, cost = timed(lambda: routes["fused"](case["fmap"], case["fmaps_ref"], case["inv_depth"], case["K"], case["ref_Ks"], case["poses"]))
                t_b, _ = timed(lambda: torch.autograd.grad((cost * case["g_" + form]).sum(), leaves))
                if i >= a.warmup:
                    fwd.append(t_f)
                    bwd.append(t_b)
            entry["fused_forward"], entry["fused_backward"] = summary(fwd), summary(bwd)
            res[f"c{C}_v{V}_{H}x{W}_{form}"] = entry
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
