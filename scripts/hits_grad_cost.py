"""What the hit pass's backward costs, on one GPU: ggr_pixel_hits_backward beside ggr_features_backward with ONE channel.

Both calls replay the same tile lists with the same front-to-back recurrence and the same butterfly; they differ in where the
per-entry gradient comes from (a staged per-Gaussian feature row against the per-pixel LDS table of K + 1 rows) — the feature
backward with one channel is the yardstick.  One step is a forward with `return_hits=K, hits_grad=True` and one feature
channel, and ONE backward of Σ gF·features + Σ G·weight + Σ Gr·rest; inside that backward each of the two library calls is
bracketed by HIP events on the backward's stream (the feature call runs first, on the scratch the forward cleared; neither
call clears anything).  Shapes: C3 (1 M Gaussians, 1920×1080, one view) and four views of C5p (480×352) in one launch set.

Prints one JSON line per (shape, K): median / min / max ms of each call over the steps, and their ratio.

    python scripts/hits_grad_cost.py --steps 12 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import GaussianRasterizer, _lib, rasterize_views  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene  # noqa: E402

DEV = "cuda:0"
CALLS = ("ggr_features_backward", "ggr_pixel_hits_backward")


def bracket(lib, name, log):
    real = getattr(lib, name)

    def timed(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(*a)
        e1.record()
        log.append((e0, e1))
        return rc

    setattr(lib, name, timed)
    return real


def make_step(shape, K, views):
    s = make_scene(**CONFIGS[shape], seed=0).to(DEV)
    P, W, H = s.means3D.shape[0], s.width, s.height
    gen = torch.Generator().manual_seed(11)
    lead = (views,) if views > 1 else ()
    G = (torch.randn(*lead, K, H, W, generator=gen) / (H * W)).to(DEV)
    Gr = (torch.randn(*lead, H, W, generator=gen) / (H * W)).to(DEV)
    gF = (torch.randn(*lead, 1, H, W, generator=gen) / (H * W)).to(DEV)
    feats = torch.rand(P, 1, generator=gen).to(DEV).requires_grad_()
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]
    m2d = torch.zeros_like(s.means3D, requires_grad=True)
    rs = s.settings()._replace(return_hits=K, hits_grad=True)
    if views > 1:
        view = torch.stack([s.viewmatrix.clone() for _ in range(views)])
        for v in range(views):
            view[v, 3, 0] += 0.05 * v
        proj = torch.stack([view[v] @ (torch.linalg.inv(s.viewmatrix) @ s.projmatrix) for v in range(views)])
        cam = torch.stack([torch.linalg.inv(view[v].T)[:3, 3] for v in range(views)])
        bg = s.bg.reshape(1, 3).expand(views, 3).contiguous()
        tf = torch.tensor([[s.tanfovx, s.tanfovy]] * views, dtype=torch.float32, device=DEV)

    def step():
        for t in leaves + [m2d, feats]:
            t.grad = None
        if views > 1:
            out = rasterize_views(leaves[0], leaves[1], view, proj, cam, bg, tf, rs, shs=leaves[2], cov3D_precomp=leaves[3],
                                  features_precomp=feats)
        else:
            out = GaussianRasterizer(rs)(means3D=leaves[0], means2D=m2d, opacities=leaves[1], shs=leaves[2],
                                         cov3D_precomp=leaves[3], features_precomp=feats)
        h = out[-1]
        torch.autograd.backward([out[3], h.weight, h.rest], [gF, G, Gr])
        return h

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C3:1,C5p:4")
    ap.add_argument("--slots", default="4,16")
    a = ap.parse_args()
    lib = _lib.load()
    logs = {n: [] for n in CALLS}
    for n in CALLS:
        bracket(lib, n, logs[n])
    for spec in a.shapes.split(","):
        shape, views = spec.split(":")
        for K in (int(k) for k in a.slots.split(",")):
            step = make_step(shape, K, int(views))
            for _ in range(a.warmup):
                h = step()
            torch.cuda.synchronize()
            for n in CALLS:
                logs[n].clear()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            ms = {n: [e0.elapsed_time(e1) for e0, e1 in logs[n]] for n in CALLS}
            assert all(len(v) == a.steps for v in ms.values())
            med = {n: statistics.median(v) for n, v in ms.items()}
            cnt = h.count.float()
            print(json.dumps({"shape": shape, "views": int(views), "K": K,
                              **{f"{n}_ms": [round(med[n], 4), round(min(ms[n]), 4), round(max(ms[n]), 4)] for n in CALLS},
                              "hits_over_features1": round(med[CALLS[1]] / med[CALLS[0]], 3),
                              "mean_count": round(float(cnt.mean()), 2), "share_count_gt_K": round(float((cnt > K).float().mean()), 3),
                              "steps": a.steps}), flush=True)
            del step, h
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
