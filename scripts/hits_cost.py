"""What the hit pass costs, on one GPU, next to the pick pass measured in the same run.

Two shapes: C3 (1 M Gaussians, 1920x1080, one view) and GGRt's launch set (C5': 1 M pixel-aligned Gaussians, 480x352, FOUR
views through `rasterize_views`).  Per shape four modes, ALTERNATED round by round, with HIP events around each block of steps
after a warm-up (as bench.py does), under torch.no_grad() (both passes are forward only):

    plain     the forward as it is
    picks     the same forward with return_picks=True: + one blend_pick launch
    hits4     the same forward with return_hits=4:  + one blend_hits launch (no memset: the kernel writes every element)
    hits16    the same forward with return_hits=16

Prints one JSON line per (shape, mode): median / min / max ms over the rounds, then the added time of each pass per shape.  No
target is set: the numbers are a record, measured against the same forward without the pass in the same run.  The pick pass is
the comparison: it walks the same lists with the same arithmetic and stores five planes at the end, where the hit pass stores
2·K planes, most of them from inside the walk.

    python scripts/hits_cost.py --steps 30 --warmup 5 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggrt_official_amd import GaussianRasterizer, rasterize_views  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene  # noqa: E402

DEV = "cuda:0"
SHAPES = {"C3": ("C3", 1), "C5p_4views": ("C5p", 4)}
MODES = {"plain": {}, "picks": dict(return_picks=True), "hits4": dict(return_hits=4), "hits16": dict(return_hits=16)}


def make_steps(shape):
    name, V = SHAPES[shape]
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    m2d = torch.zeros_like(s.means3D)
    if V == 1:
        def step(flags):
            rs = s.settings()._replace(**flags)
            return GaussianRasterizer(rs)(means3D=s.means3D, means2D=m2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)
    else:
        view = torch.stack([s.viewmatrix.clone() for _ in range(V)])
        for v in range(V):   # (a small sideways shift per view)
            view[v, 3, 0] += 0.05 * v
        proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(V)])
        cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(V)])
        bg = s.bg.reshape(1, 3).expand(V, 3).contiguous()
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * V, dtype=torch.float32, device=DEV)

        def step(flags):
            rs = s.settings()._replace(**flags)
            return rasterize_views(s.means3D, s.opacities, view, proj, cam, bg, tf, rs, shs=s.shs, cov3D_precomp=s.cov3D)
    return {m: (lambda f=f: step(f)) for m, f in MODES.items()}


def timed(step, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="C3,C5p_4views")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        steps = make_steps(shape)
        modes = list(MODES)
        with torch.no_grad():
            for m in modes:
                for _ in range(a.warmup):
                    steps[m]()
            torch.cuda.synchronize()
            ms = {m: [] for m in modes}
            for r in range(a.rounds):
                for m in (modes if r % 2 == 0 else modes[::-1]):
                    ms[m].append(timed(steps[m], a.steps))
            counts = steps["hits16"]()[-1].count
            fill = {"count_mean": round(float(counts.float().mean()), 2), "count_max": int(counts.max()),
                    "pixels_over_4": round(float((counts > 4).float().mean()), 4),
                    "pixels_over_16": round(float((counts > 16).float().mean()), 4)}
        med = {m: statistics.median(ms[m]) for m in modes}
        for m in modes:
            print(json.dumps({"shape": shape, "mode": m, "fwd_ms_median": round(med[m], 4), "min": round(min(ms[m]), 4),
                              "max": round(max(ms[m]), 4), "rounds": a.rounds, "steps": a.steps}), flush=True)
        print(json.dumps({"shape": shape, "picks_added_ms": round(med["picks"] - med["plain"], 4),
                          "hits4_added_ms": round(med["hits4"] - med["plain"], 4),
                          "hits16_added_ms": round(med["hits16"] - med["plain"], 4),
                          "hits4_over_picks_added": round((med["hits4"] - med["plain"]) / max(med["picks"] - med["plain"], 1e-9), 3),
                          "hits16_over_picks_added": round((med["hits16"] - med["plain"]) / max(med["picks"] - med["plain"], 1e-9), 3),
                          **fill}), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
