"""What the fused multi-view photometric loss costs beside the torch route it replaces, on one GPU.

GGRt's shapes: n = 13 inverse-depth maps at 378 x 504 with V = 5 reference views (pretraining) and V = 7 (finetuning); one step is
the forward plus the backward to the inverse depths and the poses.  The two routes — `fused_photometric_loss`
(csrc/photometric_loss.hip) and the float32 torch restatement of `MultiViewPhotometricDecayLoss` on the same device
(tests/photometric_loss_reference.py) — are warmed up, then timed ALTERNATELY with HIP events around each step, so that a drift of
the machine hits both.  The restatement is kinder to torch than the reference is: it keeps the clip thresholds on the device, where
the reference reads 2·n·V of them back with `float()`, and it computes the unwarped planes once, not n times.  Each route's
`torch.cuda.max_memory_allocated` over a step, above what is allocated once the inputs exist, is recorded too.  Prints one JSON line
and, with --out, writes it to a file.

    python scripts/photometric_loss_cost.py --steps 20 --warmup 3 --out profiles/photometric_loss_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_photometric_loss  # noqa: E402
from tests.photometric_loss_reference import make_photometric_case, photometric_loss_reference  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(x):
    q = statistics.quantiles(x, n=4)
    return {"ms": [round(statistics.median(x), 4), round(min(x), 4), round(max(x), 4)], "iqr_ms": round(q[2] - q[0], 4)}


def compare(routes, step, steps, warmup):
    for _ in range(warmup + 1):
        for fn in routes.values():
            step(fn)
    ms, peak = {name: [] for name in routes}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(fn)
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - before)
    for _ in range(steps):
        for name, fn in routes.items():
            ms[name].append(timed(lambda: step(fn))[0])
    out = {name: {**summary(v), "peak_bytes_above_inputs": peak[name]} for name, v in ms.items()}
    out["torch32_over_fused"] = round(out["torch32"]["ms"][0] / out["fused"]["ms"][0], 2)
    out["peak_torch32_over_fused"] = round(peak["torch32"] / max(peak["fused"], 1), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_loss_cost.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    routes = {"fused": lambda *x: fused_photometric_loss(*x).loss, "torch32": lambda *x: photometric_loss_reference(*x)["loss"]}
    for V in (5, 7):
        case = {k: v.to(device=DEV, dtype=torch.float32).contiguous() for k, v in make_photometric_case(V, 13, 378, 504, 50 + V).items()}
        inv, poses = case["inv_depths"].requires_grad_(True), case["poses"].requires_grad_(True)

        def step(fn):
            loss = fn(case["image"], case["ref_imgs"], inv, case["K"], case["ref_Ks"], poses)
            return (loss,) + torch.autograd.grad(loss.sum(), [inv, poses])

        first = {name: step(fn) for name, fn in routes.items()}
        entry = compare(routes, step, a.steps, a.warmup)
        entry["loss"] = {name: float(v[0]) for name, v in first.items()}
        entry["max_rel_difference_of_d_poses"] = float((first["fused"][2] - first["torch32"][2]).abs().max() / first["torch32"][2].abs().max())
        fwd, bwd = [], []
        for i in range(a.warmup + a.steps):
            t_f, loss = timed(lambda: routes["fused"](case["image"], case["ref_imgs"], inv, case["K"], case["ref_Ks"], poses))
            t_b, _ = timed(lambda: torch.autograd.grad(loss.sum(), [inv, poses]))
            if i >= a.warmup:
                fwd.append(t_f)
                bwd.append(t_b)
        entry["fused_forward"], entry["fused_backward"] = summary(fwd), summary(bwd)
        res[f"n13_v{V}_378x504"] = entry
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
