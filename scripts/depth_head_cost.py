"""What the fused depth head costs beside the torch route it replaces, on one GPU.

GGRt's training shape: 2 context views × 480×352 rays, s = 32 buckets, one surface, spp = 3 = 1,013,760 Gaussians.  One step is a
forward plus the backward from given gradients of depths, opacities and coordinates (fixed random weights) to the logits and to
the `to_gaussians` rows, whose first two channels `xy_raw` is a strided view of ([C, R, 2 + 7 + 3·25]).  The two routes —
`fused_depth_head` (one HIP launch each way) and the float32 torch restatement (tests/depth_head_reference.py) — get the same
uniform numbers, are warmed up, then timed ALTERNATELY with HIP events around each step, so that a drift of the machine hits both;
both modes (sampled, deterministic) are measured, use_transmittance on, opacity_exponent 2**0.5.  Prints one JSON line (median /
min / max ms of each route and mode, their ratio, the bytes the kernels must move and the rate that is of the median) and, with
--out, writes it to a file.

    python scripts/depth_head_cost.py --steps 30 --warmup 5 --out profiles/depth_head_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_depth_head  # noqa: E402
from tests.depth_head_reference import depth_head_reference  # noqa: E402

DEV = "cuda:0"
OUTPUTS = ("depths", "opacities", "coordinates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--rays", type=int, default=480 * 352)
    ap.add_argument("--buckets", type=int, default=32)
    ap.add_argument("--spp", type=int, default=3)
    ap.add_argument("--d-sh", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_head_cost.py measures on the GPU: none found")
    c, r, s, spp = a.views, a.rays, a.buckets, a.spp
    g = r * spp
    gen = torch.Generator().manual_seed(0)
    logits = (2.0 * torch.randn(c, r, 2 * s, generator=gen)).to(DEV).requires_grad_(True)
    rows = torch.randn(c, r, 2 + 7 + 3 * a.d_sh, generator=gen).to(DEV).requires_grad_(True)
    common = dict(ray_xy=torch.rand(r, 2, generator=gen).to(DEV), near=torch.linspace(0.7, 1.1, c).to(DEV),
                  far=torch.full((c,), 80.0).to(DEV), image_shape=(352, 480), num_surfaces=1, samples_per_ray=spp,
                  use_transmittance=True, opacity_exponent=2 ** 0.5)
    u = torch.rand(c, r, 1, spp, generator=gen).to(DEV)
    weights = [torch.randn(c, g, *tail, generator=gen).to(DEV) for tail in ((), (), (2,))]

    def step(fn, deterministic):
        """forward + backward of the depth head alone, between two events: the outputs' gradients are the weights"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(logits=logits, xy_raw=rows[..., :2], deterministic=deterministic, u=None if deterministic else u, **common)
        out = out if isinstance(out, dict) else dict(depths=out.depths, opacities=out.opacities, coordinates=out.coordinates, index=out.index)
        grads = torch.autograd.grad([out[k] for k in OUTPUTS], [logits, rows], weights)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out["index"], grads

    routes = {"fused": fused_depth_head, "torch32": depth_head_reference}
    res = {"gaussians": c * g, "views": c, "rays": r, "buckets": s, "spp": spp, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    # bytes the two launches must move: forward reads the logits, xy_raw (8 B per ray, in 128 B lines of the rows) and u, writes
    # depth, opacity, coords, index; backward reads the logits, index, xy_raw and the three gradients and writes dL/dlogits and
    # the dense dL/dxy_raw
    moved = c * r * (8 * s + 8) * 2 + c * g * (4 + 16) + c * g * (4 + 16) + c * r * (8 * s + 8)
    for deterministic in (False, True):
        mode = "deterministic" if deterministic else "sampled"
        first = {n: step(fn, deterministic) for n, fn in routes.items()}     # (also the first warm-up)
        same = float((first["fused"][1].long() == first["torch32"][1]).float().mean())
        agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(first["fused"][2], first["torch32"][2])]
        del first
        for _ in range(a.warmup):
            for fn in routes.values():
                step(fn, deterministic)
        ms = {n: [] for n in routes}
        for _ in range(a.steps):
            for n, fn in routes.items():
                ms[n].append(step(fn, deterministic)[0])
        med = {n: statistics.median(v) for n, v in ms.items()}
        res[mode] = {**{n: {"ms": [round(med[n], 4), round(min(v), 4), round(max(v), 4)],
                            "iqr_ms": round(statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0], 4)} for n, v in ms.items()},
                     "torch32_over_fused": round(med["torch32"] / med["fused"], 2),
                     "fused_GB_per_s_of_step": round(moved / med["fused"] / 1e6, 1),
                     "share_of_rows_with_the_same_index": same, "max_rel_difference_of_gradients": {"logits": agree[0], "rows": agree[1]}}
    res["kernel_bytes_moved"] = int(moved)
    line = json.dumps(res)
    print(line, flush=True)
    for mode in ("sampled", "deterministic"):
        if not res[mode]["fused"]["ms"][0] < res[mode]["torch32"]["ms"][0]:
            raise SystemExit(f"{mode}: the fused route is not faster than the torch route")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
