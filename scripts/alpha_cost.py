"""What the accumulated-opacity output (GaussianRasterizationSettings.return_alpha) costs, on one GPU.

Times forward + backward of C3 (1 M Gaussians, 1920x1080, one view) and of GGRt's 4-view training shape (C5': 1 M pixel-aligned
Gaussians, 4 views of 480x352 in one launch set): without alpha (an upstream gradient for the colour) and with it (upstream
gradients for the colour and for alpha, handed to autograd directly — no loss kernels of torch's — so that the backward runs
its alpha instance), ALTERNATED round by round, with HIP events around each step after a warm-up (as bench.py does).  Prints one JSON line per (shape, mode): median / min / max ms over the rounds.

    python scripts/alpha_cost.py --steps 50 --warmup 10 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import GaussianRasterizer, rasterize_views  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene, upstream_gradient  # noqa: E402

DEV = "cuda:0"


def one_view(name):
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    dL = upstream_gradient(s.width, s.height, device=DEV)
    g = upstream_gradient(s.width, s.height, seed=1, device=DEV)[0]
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]
    m2d = torch.zeros_like(s.means3D, requires_grad=True)

    def step(alpha_on):
        for t in leaves + [m2d]:
            t.grad = None
        rs = s.settings()._replace(return_alpha=alpha_on)
        out = GaussianRasterizer(rs)(means3D=leaves[0], means2D=m2d, opacities=leaves[1], shs=leaves[2],
                                     cov3D_precomp=leaves[3])
        if alpha_on:
            torch.autograd.backward([out[0], out[3]], [dL, g])
        else:
            out[0].backward(dL)
    return step


def four_views(name, V=4):
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    view = torch.stack([s.viewmatrix.clone() for _ in range(V)])
    for v in range(V):
        view[v, 3, 0] += 0.02 * v
    proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(V)])
    cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(V)])
    bg = s.bg.reshape(1, 3).expand(V, 3).contiguous()
    tf = torch.tensor([[s.tanfovx, s.tanfovy]] * V, dtype=torch.float32, device=DEV)
    dL = torch.stack([upstream_gradient(s.width, s.height, seed=v, device=DEV) for v in range(V)])
    g = torch.stack([upstream_gradient(s.width, s.height, seed=10 + v, device=DEV)[0] for v in range(V)])
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]

    def step(alpha_on):
        for t in leaves:
            t.grad = None
        rs = s.settings()._replace(return_alpha=alpha_on)
        out = rasterize_views(leaves[0], leaves[1], view, proj, cam, bg, tf, rs, shs=leaves[2], cov3D_precomp=leaves[3])
        if alpha_on:
            torch.autograd.backward([out[0], out[3]], [dL, g])
        else:
            out[0].backward(dL)
    return step


def timed(step, alpha_on, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        step(alpha_on)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for label, make in (("C3", lambda: one_view("C3")), ("C5p_4views", lambda: four_views("C5p"))):
        step = make()
        for on in (False, True):
            for _ in range(a.warmup):
                step(on)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for r in range(a.rounds):
            for on in ((False, True) if r % 2 == 0 else (True, False)):
                ms[on].append(timed(step, on, a.steps))
        for on in (False, True):
            print(json.dumps({"shape": label, "return_alpha": on, "fwd_bwd_ms_median": round(statistics.median(ms[on]), 4),
                              "min": round(min(ms[on]), 4), "max": round(max(ms[on]), 4), "rounds": a.rounds,
                              "steps": a.steps}), flush=True)
        del step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
