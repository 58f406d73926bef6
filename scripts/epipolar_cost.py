"""What the fused epipolar sampler costs beside the torch route it replaces, on one GPU.

GGRt's training shape: b = 1, v = 2 context views, 120 × 88 rays (the 480 × 352 frame after `downscale: 4`), s = 32 samples,
c = 128 channels: the key/value tensor `features` is 86.5 M floats; v = 3 at the same size is measured too.  One step is a
forward plus the backward from a given gradient of `features` (fixed random weights) to the feature maps.  The two routes —
`fused_epipolar_sampler` (csrc/epipolar.hip) and the float32 torch restatement (tests/epipolar_reference.py: the same stage with
grid_sample, without the reference's lstsq) — are warmed up, then timed ALTERNATELY with HIP events around each step, so that a
drift of the machine hits both.  Prints one JSON line (median / min / max ms of each route and shape, their ratio, the bytes the
fused route must move — every output written once, the feature maps read once, and the mirror of that for the backward — and
the share of the HBM rate that is of the median step) and, with --out, writes it to a file.

    python scripts/epipolar_cost.py --steps 20 --warmup 3 --out profiles/epipolar_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_epipolar_sampler  # noqa: E402
from tests.epipolar_reference import epipolar_reference, make_case  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12      # the MI355X's specified HBM3E rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=88)
    ap.add_argument("--width", type=int, default=120)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epipolar_cost.py measures on the GPU: none found")
    h, w, s, c = a.height, a.width, a.samples, a.channels
    res = {"height": h, "width": w, "samples": s, "channels": c, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    for v in a.views:
        cams = make_case(1, v, 3, 4, 1, 4, 7, "default")          # (cameras of the tests' default family; the maps are drawn here)
        gen = torch.Generator().manual_seed(v)
        images = torch.randn(1, v, c, h, w, generator=gen).to(DEV).requires_grad_(True)
        args = {k: cams[k].to(device=DEV, dtype=torch.float32) for k in ("extrinsics", "intrinsics", "near", "far")}
        pairs = v * (v - 1) * h * w
        weights = torch.randn(1, v, v - 1, h * w, s, c, generator=gen).to(DEV)

        def step(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(images, num_samples=s, **args)
            features, valid = (out["features"], out["valid"]) if isinstance(out, dict) else (out.features, out.valid)
            (g,) = torch.autograd.grad([features], [images], [weights])
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), features, valid, g

        routes = {"fused": fused_epipolar_sampler, "torch32": epipolar_reference}
        first = {n: step(fn) for n, fn in routes.items()}          # (also the first warm-up)
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
        agree = dict(valid_equal_share=float((first["fused"][2] == first["torch32"][2]).float().mean()),
                     valid_share=float(first["fused"][2].float().mean()),
                     max_rel_difference_of_features=rel(first["fused"][1], first["torch32"][1]),
                     max_rel_difference_of_gradient=rel(first["fused"][3], first["torch32"][3]))
        del first
        for _ in range(a.warmup):
            for fn in routes.values():
                step(fn)
        ms = {n: [] for n in routes}
        for _ in range(a.steps):
            for n, fn in routes.items():
                ms[n].append(step(fn)[0])
        med = {n: statistics.median(x) for n, x in ms.items()}
        # forward: features + 3 xy + depth per sample, valid + segment per pair-ray, the per-ray outputs, the maps read once;
        # backward: dL/dfeatures read once, dL/dimages written once
        per_sample, maps = 4 * (c + 7), 4 * v * c * h * w
        moved = pairs * (s * per_sample + 17) + v * h * w * 32 + maps + pairs * s * c * 4 + maps
        res[f"views_{v}"] = {**{n: {"ms": [round(med[n], 4), round(min(x), 4), round(max(x), 4)],
                                    "iqr_ms": round(statistics.quantiles(x, n=4)[2] - statistics.quantiles(x, n=4)[0], 4)} for n, x in ms.items()},
                             "torch32_over_fused": round(med["torch32"] / med["fused"], 2), "fused_bytes_to_move": int(moved),
                             "fused_GB_per_s_of_step": round(moved / med["fused"] / 1e6, 1),
                             "fused_share_of_hbm_rate": round(moved / (med["fused"] * 1e-3) / HBM_BYTES_PER_S, 4), "pair_rays": pairs, **agree}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
