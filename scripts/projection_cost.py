"""What the projection pass costs, on one GPU: projection_unpack and projection_seed beside the streaming yardstick.

One step is a forward with `return_projection=True` at C3's Gaussians (1 M (view, Gaussian) pairs, 1920×1080, one view) and ONE
backward of a loss over all five projection fields; inside them `ggr_projection` and `ggr_projection_backward` are each bracketed
by HIP events on their stream.  The backward call of a first backward adds into the scratch the forward cleared (the ADD form);
`--second` also times a second backward over the same forward, whose scratch is not clear (the form that writes whole records).
The yardstick is `ggr_debug_copy` (a float4 copy, what bench.py quotes as the streaming ceiling) over the SAME number of bytes
moved, read + written: per pair the unpack kernel reads 52 B (two float4 of the splat record, the float4 colour, the radius) and
writes 41 B; the seeding kernel reads 44 B (radius + five gradient arrays) and read-modify-writes 40 B of the record (ADD) or
writes its 64 B.  Prints one JSON line: median / min / max ms of each call, the copy's, and the ratios.

    python scripts/projection_cost.py --steps 12 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import GaussianRasterizer, _lib  # noqa: E402
from ggrt_official_amd.synthetic import CONFIGS, make_scene  # noqa: E402

DEV = "cuda:0"
CALLS = ("ggr_projection", "ggr_projection_backward")
BYTES = {"ggr_projection": 52 + 41, "ggr_projection_backward": 44 + 80, "second_backward": 44 + 64}


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


def copy_ms(lib, moved, reps):
    """median ms of the float4 copy that moves `moved` bytes (half read, half written)"""
    n = (moved // 2) // 16 * 16
    src = torch.empty(n, dtype=torch.uint8, device=DEV).random_(0, 255)
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert lib.ggr_debug_copy(src.data_ptr(), dst.data_ptr(), n, 0, stream) == 0
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--second", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    logs = {n: [] for n in CALLS}
    for n in CALLS:
        bracket(lib, n, logs[n])
    s = make_scene(**CONFIGS[a.shape], seed=0).to(DEV)
    P = s.means3D.shape[0]
    gen = torch.Generator().manual_seed(13)
    g = [(torch.randn(P, *tail, generator=gen) / P).to(DEV) for tail in ((2,), (), (3,), (), (3,))]
    leaves = [t.clone().requires_grad_() for t in (s.means3D, s.opacities, s.shs, s.cov3D)]
    m2d = torch.zeros_like(s.means3D, requires_grad=True)
    rast = GaussianRasterizer(s.settings()._replace(return_projection=True))

    def step():
        for t in leaves + [m2d]:
            t.grad = None
        p = rast(means3D=leaves[0], means2D=m2d, opacities=leaves[1], shs=leaves[2], cov3D_precomp=leaves[3])[-1]
        torch.autograd.backward(list(p[:5]), g, retain_graph=a.second)
        if a.second:
            torch.autograd.backward(list(p[:5]), g)
        return p

    for _ in range(a.warmup):
        p = step()
    torch.cuda.synchronize()
    for n in CALLS:
        logs[n].clear()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = {n: [e0.elapsed_time(e1) for e0, e1 in logs[n]] for n in CALLS}
    if a.second:   # the backward calls alternate: first (ADD), second (whole records)
        ms["second_backward"] = ms["ggr_projection_backward"][1::2]
        ms["ggr_projection_backward"] = ms["ggr_projection_backward"][0::2]
    out = {"shape": a.shape, "pairs": P, "valid_share": round(float(p.valid.float().mean()), 3), "steps": a.steps}
    for n, v in ms.items():
        assert len(v) == a.steps
        med, moved = statistics.median(v), BYTES[n] * P
        c = copy_ms(lib, moved, a.steps)
        out[n] = {"ms": [round(med, 4), round(min(v), 4), round(max(v), 4)], "bytes_moved": moved, "copy_ms": round(c, 4),
                  "over_copy": round(med / c, 2), "GB_per_s": round(moved / med / 1e6, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
