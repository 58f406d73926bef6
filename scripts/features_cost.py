"""What K rendered feature channels cost, on one GPU: the feature pass against the ceil(K/3)-call loop it replaces.

Times forward + backward at C3 (1 M Gaussians, 1920x1080, one view) and at GGRt's 480x352 shape (C5': 1 M pixel-aligned
Gaussians, one view), for K = 4 and K = 16, three ways, ALTERNATED round by round, with HIP events around each step after a
warm-up (as bench.py does); upstream gradients are handed to autograd directly (no loss kernels of torch's):

    plain   one colour render (SH colours), no features                         — the baseline a host pays anyway
    pass    the same render with features_precomp [P,K]: colour + K channels    — ONE call
    loop    the same colour render + ceil(K/3) more calls with colors_precomp = 3-channel slices, bg = 0 — the only route
            without the feature pass (every call repeats preprocess, sort, list build, blend and the whole backward)

Prints one JSON line per (shape, K, mode): median / min / max ms over the rounds, then per (shape, K) the ratios
loop/pass and (pass − plain)/(loop − plain), the cost of the K channels alone.

    python scripts/features_cost.py --steps 30 --warmup 5 --rounds 5
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


def make_steps(name, K):
    s = make_scene(**CONFIGS[name], seed=0).to(DEV)
    P, W, H = s.means3D.shape[0], s.width, s.height
    dL = upstream_gradient(W, H, device=DEV)
    gF = torch.cat([upstream_gradient(W, H, seed=1 + i, device=DEV) for i in range((K + 2) // 3)])[:K].contiguous()
    feats = torch.rand(P, K, generator=torch.Generator().manual_seed(5)).to(DEV)
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]
    f_leaf = feats.clone().requires_grad_()
    slices, g_slices = [], []
    for k0 in range(0, K, 3):
        n = min(3, K - k0)
        sl, g = torch.zeros(P, 3, device=DEV), torch.zeros(3, H, W, device=DEV)
        sl[:, :n], g[:n] = feats[:, k0:k0 + n], gF[k0:k0 + n]
        slices.append(sl.requires_grad_())
        g_slices.append(g)
    m2d = torch.zeros_like(s.means3D, requires_grad=True)
    rs = s.settings()
    rs0 = rs._replace(bg=torch.zeros(3, device=DEV))

    def clear():
        for t in leaves + [m2d, f_leaf] + slices:
            t.grad = None

    def colour(**kw):
        return GaussianRasterizer(rs)(means3D=leaves[0], means2D=m2d, opacities=leaves[1], shs=leaves[2],
                                      cov3D_precomp=leaves[3], **kw)

    def plain():
        clear()
        colour()[0].backward(dL)

    def one_pass():
        clear()
        out = colour(features_precomp=f_leaf)
        torch.autograd.backward([out[0], out[-1]], [dL, gF])

    def loop():
        clear()
        colour()[0].backward(dL)
        for sl, g in zip(slices, g_slices):
            GaussianRasterizer(rs0)(means3D=leaves[0], means2D=m2d, opacities=leaves[1], colors_precomp=sl,
                                    cov3D_precomp=leaves[3])[0].backward(g)

    return {"plain": plain, "pass": one_pass, "loop": loop}


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
    ap.add_argument("--shapes", default="C3,C5p")
    ap.add_argument("--channels", default="4,16")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        for K in (int(k) for k in a.channels.split(",")):
            steps = make_steps(name, K)
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
                print(json.dumps({"shape": name, "K": K, "mode": m, "fwd_bwd_ms_median": round(med[m], 4),
                                  "min": round(min(ms[m]), 4), "max": round(max(ms[m]), 4), "rounds": a.rounds,
                                  "steps": a.steps}), flush=True)
            print(json.dumps({"shape": name, "K": K, "loop_over_pass": round(med["loop"] / med["pass"], 3),
                              "added_ms_pass": round(med["pass"] - med["plain"], 4),
                              "added_ms_loop": round(med["loop"] - med["plain"], 4),
                              "added_pass_over_added_loop": round((med["pass"] - med["plain"]) / (med["loop"] - med["plain"]), 3)}),
                  flush=True)
            del steps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
