"""What the distortion pass costs, on one GPU, next to the feature pass at K = 4 for scale.

At C3 (1 M Gaussians, 1920x1080, one view; --shapes for others) three renders — plain (SH colours), with return_distortion,
with features_precomp [P,4] — are timed forward-only (torch.no_grad) and forward + backward, ALTERNATED round by round, with
HIP events around each step after a warm-up (as bench.py does); upstream gradients are handed to autograd directly.  Per pass:
    forward ms  = forward-only(with) − forward-only(plain)
    backward ms = [fwd+bwd(with) − fwd+bwd(plain)] − forward ms     (the training forward also stores the per-pixel totals)
Prints one JSON line per (shape, mode) with median / min / max ms over the rounds, then one line of the differences.

    python scripts/distortion_cost.py --steps 30 --warmup 5 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import GaussianRasterizer  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene, upstream_gradient  # noqa: E402

DEV = "cuda:0"
K = 4


def make_steps(name):
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    P, W, H = s.means3D.shape[0], s.width, s.height
    dL = upstream_gradient(W, H, device=DEV)
    gQ = upstream_gradient(W, H, seed=7, device=DEV)[0].contiguous()
    gF = torch.cat([upstream_gradient(W, H, seed=1 + i, device=DEV) for i in range(2)])[:K].contiguous()
    feats = torch.rand(P, K, generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_()
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]
    m2d = torch.zeros_like(s.means3D, requires_grad=True)
    rs = s.settings()

    def render(settings, **kw):
        for t in leaves + [m2d, feats]:
            t.grad = None
        return GaussianRasterizer(settings)(means3D=leaves[0], means2D=m2d, opacities=leaves[1], shs=leaves[2],
                                            cov3D_precomp=leaves[3], **kw)

    def fwd(fn):
        def step():
            with torch.no_grad():
                fn()
        return step

    plain = lambda: render(rs)
    dist = lambda: render(rs._replace(return_distortion=True))
    feat = lambda: render(rs, features_precomp=feats)
    return {
        "fwd_plain": fwd(plain), "fwd_distortion": fwd(dist), "fwd_features4": fwd(feat),
        "step_plain": lambda: plain()[0].backward(dL),
        "step_distortion": lambda: (lambda o: torch.autograd.backward([o[0], o[-1]], [dL, gQ]))(dist()),
        "step_features4": lambda: (lambda o: torch.autograd.backward([o[0], o[-1]], [dL, gF]))(feat()),
    }


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
    ap.add_argument("--shapes", default="C3")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        steps = make_steps(name)
        modes = list(steps)
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
            print(json.dumps({"shape": name, "mode": m, "ms_median": round(med[m], 4), "min": round(min(ms[m]), 4),
                              "max": round(max(ms[m]), 4), "rounds": a.rounds, "steps": a.steps}), flush=True)
        out = {"shape": name}
        for p in ("distortion", "features4"):
            f = med[f"fwd_{p}"] - med["fwd_plain"]
            out[f"{p}_forward_ms"] = round(f, 4)
            out[f"{p}_backward_ms"] = round(med[f"step_{p}"] - med["step_plain"] - f, 4)
        print(json.dumps(out), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
