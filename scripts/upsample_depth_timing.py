"""What the fused convex depth upsampling costs beside the torch route it replaces, on one GPU.

GGRt's shape: 48 x 63 cells (378 x 504 at 1/8) at ratio 8, `up` 384 x 504 resized to 378 x 504, followed by
`disp_to_depth(..., 0.1, 100)`; N = 4 is the four predictions of one `DepthPoseNet.forward` upsampled in one call, N = 1 a single
prediction.  One step is the forward plus the backward to the depth and the mask.  The two routes — `fused_upsample_depth`
(csrc/upsample_depth.hip) and a float32 torch route on the same device — are warmed up, then timed ALTERNATELY with HIP events around
each step, so that a drift of the machine hits both.  The torch route is the restatement's convex combination
(tests/upsample_depth_reference.py: a softmax over the taps, nine shifted views of the padded map, a broadcast multiply and a sum, a
permute copy) followed by `F.interpolate(..., align_corners=True)` and the affine map, as the reference resizes.  For N = 4 the torch
route is timed both as one stacked call and as the four calls of one map each that the reference issues.  Each route's
`torch.cuda.max_memory_allocated` over a step, above what is allocated once the inputs exist, is recorded too.  Prints one JSON line
and, with --out, writes it to a file.

    python scripts/upsample_depth_timing.py --steps 50 --warmup 10 --out profiles/upsample_depth_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_upsample_depth  # noqa: E402
from tests.upsample_depth_reference import INPUTS, convex_upsample, make_upsample_case  # noqa: E402

DEV = "cuda:0"
H, W, R, SIZE, DISP_RANGE = 48, 63, 8, (378, 504), (0.1, 100.0)


def torch_route(depth, mask):
    up = F.interpolate(convex_upsample(depth, mask, R), size=SIZE, mode="bilinear", align_corners=True)
    return 1.0 / DISP_RANGE[1] + (1.0 / DISP_RANGE[0] - 1.0 / DISP_RANGE[1]) * up


def torch_route_per_map(depth, mask):
    return torch.cat([torch_route(depth[n:n + 1], mask[n:n + 1]) for n in range(depth.shape[0])], 0)


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
    for name in routes:
        if name != "fused":
            out[name + "_over_fused"] = round(out[name]["ms"][0] / out["fused"]["ms"][0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_depth_timing.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for N in (4, 1):
        case = {k: v.to(device=DEV, dtype=torch.float32).contiguous() for k, v in make_upsample_case(N, H, W, R, SIZE, 70 + N).items()}
        leaves = [case[k].requires_grad_(True) for k in INPUTS]
        routes = {"fused": lambda d, m: fused_upsample_depth(d, m, ratio=R, image_size=SIZE, disp_range=DISP_RANGE), "torch32": torch_route}
        if N > 1:
            routes["torch32_per_map"] = torch_route_per_map

        def step(fn):
            out = fn(case["depth"], case["mask"])
            return (out,) + torch.autograd.grad((out * case["g"]).sum(), leaves)

        first = {name: step(fn) for name, fn in routes.items()}
        entry = compare(routes, step, a.steps, a.warmup)
        entry["max_rel_difference"] = {k: float((x.detach() - y.detach()).abs().max() / y.detach().abs().max()) for k, x, y in zip(("out",) + INPUTS, first["fused"], first["torch32"])}
        fwd, bwd = [], []
        for i in range(a.warmup + a.steps):
            t_f, out = timed(lambda: routes["fused"](case["depth"], case["mask"]))
            t_b, _ = timed(lambda: torch.autograd.grad((out * case["g"]).sum(), leaves))
            if i >= a.warmup:
                fwd.append(t_f)
                bwd.append(t_b)
        entry["fused_forward"], entry["fused_backward"] = summary(fwd), summary(bwd)
        entry["bytes"] = {"mask": N * 9 * R * R * H * W * 4, "up": N * R * R * H * W * 4, "out": N * SIZE[0] * SIZE[1] * 4}
        res[f"n{N}_{H}x{W}_r{R}_to_{SIZE[0]}x{SIZE[1]}"] = entry
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
