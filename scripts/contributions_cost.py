"""What the contribution pass costs, on one GPU: forward-only time with and without `return_contributions`.

Two shapes: C3 (1 M Gaussians, 1920x1080, one view) and GGRt's launch set (C5': 1 M pixel-aligned Gaussians, 480x352, FOUR
views through `rasterize_views`).  Per shape two modes, ALTERNATED round by round, with HIP events around each block of steps
after a warm-up (as bench.py does), under torch.no_grad() (the pass is forward only):

    plain   the forward as it is
    pass    the same forward with return_contributions=True: + three memsets and one blend_contrib launch

Prints one JSON line per (shape, mode): median / min / max ms over the rounds, then the added time per shape.

`--profile` then starts ONE child per shape under `rocprofv3 --kernel-trace --stats` (the child runs `--trace SHAPE`: warm-up
and `--steps` forwards with the pass) and reports the average kernel time of blend_contrib next to blend_fwd's on the same
frames — the pass walks the same lists as the colour blend, with less arithmetic per pair and up to three atomics per
(tile, entry).

    python scripts/contributions_cost.py --steps 30 --warmup 5 --rounds 5 --profile
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


def make_steps(shape):
    name, V = SHAPES[shape]
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    m2d = torch.zeros_like(s.means3D)
    if V == 1:
        def step(on):
            rs = s.settings()._replace(return_contributions=on)
            return GaussianRasterizer(rs)(means3D=s.means3D, means2D=m2d, opacities=s.opacities, shs=s.shs, cov3D_precomp=s.cov3D)
    else:
        view = torch.stack([s.viewmatrix.clone() for _ in range(V)])
        for v in range(V):   # (a small sideways shift per view)
            view[v, 3, 0] += 0.05 * v
        proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(V)])
        cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(V)])
        bg = s.bg.reshape(1, 3).expand(V, 3).contiguous()
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * V, dtype=torch.float32, device=DEV)

        def step(on):
            rs = s.settings()._replace(return_contributions=on)
            return rasterize_views(s.means3D, s.opacities, view, proj, cam, bg, tf, rs, shs=s.shs, cov3D_precomp=s.cov3D)
    return {"plain": lambda: step(False), "pass": lambda: step(True)}


def timed(step, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def trace(shape, steps, warmup):
    """the child of --profile: forwards with the pass, nothing else"""
    step = make_steps(shape)["pass"]
    with torch.no_grad():
        for _ in range(warmup + steps):
            step()
    torch.cuda.synchronize()


def profile(shape, steps, warmup):
    """average kernel time (µs) of blend_contrib and blend_fwd over one traced child run"""
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
                    for key in ("blend_contrib_kernel", "blend_fwd"):
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
    ap.add_argument("--trace", default=None, help="(internal) run only forwards with the pass for this shape")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.steps, a.warmup)
        return
    for shape in a.shapes.split(","):
        steps = make_steps(shape)
        modes = list(steps)
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
        print(json.dumps({"shape": shape, "added_ms": round(med["pass"] - med["plain"], 4),
                          "pass_over_plain": round(med["pass"] / med["plain"], 3)}), flush=True)
        del steps
        torch.cuda.empty_cache()
    if a.profile:
        torch.cuda.synchronize()
        for shape in a.shapes.split(","):
            print(json.dumps(profile(shape, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
