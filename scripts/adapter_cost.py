"""What the fused Gaussian adapter costs beside the torch route it replaces, on one GPU.

GGRt's training shape: 2 context views × 480×352 rays × spp = 3 = 1,013,760 Gaussians, d_sh = 25.  One step is a forward plus
the backward of a loss over all four outputs (fixed random weights), with gradients for raw, depth, extrinsics, intrinsics and
sh_transform.  The two routes — `fused_gaussian_adapter` (one HIP launch each way plus the tiny per-camera torch ops) and the
float32 torch restatement (tests/adapter_reference.py: the arithmetic of GaussianAdapter.forward, sh_transform given) — are warmed
up, then timed ALTERNATELY with HIP events around each step, so that a drift of the machine hits both.  Prints one JSON line
(median / min / max ms of each route, their ratio, the bytes the kernels must move and the rate that is of the median) and, with
--out, writes it to a file.

    python scripts/adapter_cost.py --steps 30 --warmup 5 --out profiles/adapter_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_gaussian_adapter  # noqa: E402
from tests.adapter_reference import adapter_reference, make_case  # noqa: E402

DEV = "cuda:0"
OUTPUTS = ("means", "scales", "rotations", "harmonics")
LEAVES = ("raw_gaussians", "depths", "extrinsics", "intrinsics", "sh_transform")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--rays", type=int, default=480 * 352)
    ap.add_argument("--spp", type=int, default=3)
    ap.add_argument("--d-sh", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapter_cost.py measures on the GPU: none found")
    g = a.rays * a.spp
    case = make_case(a.views, g, a.spp, a.d_sh, seed=0, image_shape=(352, 480))
    args = {k: (v.to(device=DEV, dtype=torch.float32) if torch.is_tensor(v) else v) for k, v in case.items()}
    for k in LEAVES:
        args[k].requires_grad_(True)
    gen = torch.Generator().manual_seed(1)
    p = a.views * g
    weights = {k: torch.randn(p, *tail, generator=gen).to(DEV) for k, tail in
               zip(OUTPUTS, ((3,), (3,), (4,), (3, a.d_sh)))}

    def step(fn):
        out = fn(**args)
        out = out if isinstance(out, dict) else dict(means=out.means, scales=out.scales, rotations=out.rotations, harmonics=out.harmonics)
        loss = sum((out[k] * weights[k]).sum() for k in OUTPUTS)
        return torch.autograd.grad(loss, [args[k] for k in LEAVES])

    def adapter_only(fn):
        """forward + backward of the adapter alone: the loss's own products stay outside the events (they are the same torch ops
        for both routes): the outputs' gradients are the weights"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(**args)
        out = out if isinstance(out, dict) else dict(means=out.means, scales=out.scales, rotations=out.rotations, harmonics=out.harmonics)
        torch.autograd.grad([out[k] for k in OUTPUTS], [args[k] for k in LEAVES], [weights[k] for k in OUTPUTS])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    routes = {"fused": fused_gaussian_adapter, "torch32": adapter_reference}
    grads = {n: step(fn) for n, fn in routes.items()}     # (also the first warm-up; and the two routes compute the same)
    agree = {k: float((x - y).abs().max() / y.abs().max()) for k, x, y in zip(LEAVES, grads["fused"], grads["torch32"])}
    del grads
    for _ in range(a.warmup):
        for fn in routes.values():
            adapter_only(fn)
    ms = {n: [] for n in routes}
    for _ in range(a.steps):
        for n, fn in routes.items():
            ms[n].append(adapter_only(fn))
    w = 7 + 3 * a.d_sh
    # bytes the two launches must move per Gaussian: forward reads depth, coords and 1/spp of a raw row, writes means, scales,
    # quats, harmonics; backward reads those inputs and the four gradients, writes dL/ddepth (dL/dcoords is not asked for
    # here) and 1/spp of a dL/draw row
    out_b = 4 * (3 + 3 + 4 + 3 * a.d_sh)
    moved = p * (12 + 4 * w / a.spp + out_b) + p * (12 + 4 * w / a.spp + out_b + 4 + 4 * w / a.spp)
    med = {n: statistics.median(v) for n, v in ms.items()}
    res = {"gaussians": p, "views": a.views, "spp": a.spp, "d_sh": a.d_sh, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           **{n: {"ms": [round(med[n], 4), round(min(v), 4), round(max(v), 4)],
                  "iqr_ms": round(statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0], 4)} for n, v in ms.items()},
           "torch32_over_fused": round(med["torch32"] / med["fused"], 2), "kernel_bytes_moved": int(moved),
           "fused_GB_per_s_of_step": round(moved / med["fused"] / 1e6, 1), "max_rel_difference_of_gradients": agree}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
