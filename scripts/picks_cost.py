"""What the pick pass costs, on one GPU, next to the contribution pass measured in the same run.

Two shapes: C3 (1 M Gaussians, 1920x1080, one view) and GGRt's launch set (C5': 1 M pixel-aligned Gaussians, 480x352, FOUR
views through `rasterize_views`).  Per shape three modes, ALTERNATED round by round, with HIP events around each block of steps
after a warm-up (as bench.py does), under torch.no_grad() (both passes are forward only):

    plain     the forward as it is
    contrib   the same forward with return_contributions=True: + three memsets and one blend_contrib launch
    picks     the same forward with return_picks=True: + one blend_pick launch (no memset: the kernel writes every pixel)

Prints one JSON line per (shape, mode): median / min / max ms over the rounds, then the added time of both passes per shape.
The yardstick of the pick pass is the contribution pass of the SAME run: it walks the same lists with the same arithmetic and
has no butterflies, no LDS tables and no atomics.

`--profile` then starts ONE child per shape under `rocprofv3 --kernel-trace --stats` (the child runs `--trace SHAPE`: warm-up
and `--steps` forwards with both passes) and reports the average kernel time of blend_pick next to blend_contrib's and
blend_fwd's on the same frames.

    python scripts/picks_cost.py --steps 30 --warmup 5 --rounds 5 --profile
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggrt_official_amd import GaussianRasterizer, rasterize_views  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene  # noqa: E402

DEV = "cuda:0"
SHAPES = {"C3": ("C3", 1), "C5p_4views": ("C5p", 4)}
MODES = {"plain": {}, "contrib": dict(return_contributions=True), "picks": dict(return_picks=True)}   # the timed modes
TRACED = dict(return_contributions=True, return_picks=True)   # what the --profile child runs: both passes on the same frames
KERNELS = ("blend_pick_kernel", "blend_contrib_kernel", "blend_fwd")


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
    return {m: (lambda f=f: step(f)) for m, f in MODES.items()}, lambda: step(TRACED)


def timed(step, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def trace(shape, steps, warmup):
    """the child of --profile: forwards with both passes, nothing else"""
    _timed, step = make_steps(shape)
    with torch.no_grad():
        for _ in range(warmup + steps):
            step()
    torch.cuda.synchronize()


def profile(shape, steps, warmup):
    """average kernel time (µs) of blend_pick, blend_contrib and blend_fwd over one traced child run"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--trace", shape, "--steps", str(steps), "--warmup", str(warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if r.returncode != 0:
            return {"shape": shape, "profile_error": r.stdout[-400:]}
        out = {"shape": shape}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    nm = row.get("Name", "")
                    for key in KERNELS:
                        if key in nm and "AverageNs" in row:
                            out[key + "_avg_us"] = round(float(row["AverageNs"]) / 1e3, 2)
                            out[key + "_calls"] = int(row.get("Calls", 0))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="C3,C5p_4views")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--trace", default=None, help="(internal) run only forwards with both passes for this shape")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.steps, a.warmup)
        return
    for shape in a.shapes.split(","):
        steps, _traced = make_steps(shape)
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
        med = {m: statistics.median(ms[m]) for m in modes}
        for m in modes:
            print(json.dumps({"shape": shape, "mode": m, "fwd_ms_median": round(med[m], 4), "min": round(min(ms[m]), 4),
                              "max": round(max(ms[m]), 4), "rounds": a.rounds, "steps": a.steps}), flush=True)
        print(json.dumps({"shape": shape, "contrib_added_ms": round(med["contrib"] - med["plain"], 4),
                          "picks_added_ms": round(med["picks"] - med["plain"], 4),
                          "picks_over_contrib_added": round((med["picks"] - med["plain"]) / max(med["contrib"] - med["plain"], 1e-9), 3)}),
              flush=True)
        del steps, _traced
        torch.cuda.empty_cache()
    if a.profile:
        torch.cuda.synchronize()
        for shape in a.shapes.split(","):
            print(json.dumps(profile(shape, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
