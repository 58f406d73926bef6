"""What the fused image loss costs beside the torch route it replaces, on one GPU.

Two shapes: GGRt's training step, [2, 3, 352, 480] with a mask — forward of 0.8·mse + 0.2·(1 − ssim) plus the backward to the
rendered image — and the LLFF evaluation frame, [1, 3, 320, 448] without one — forward only, ssim and psnr under `no_grad`, as the
evaluation loop calls them.  The two routes — `fused_image_loss` (csrc/image_loss.hip) and the literal float32 torch restatement of
the reference's `img2mse` and `ssim` on the same device (tests/image_loss_reference.py: five depthwise 11 × 11 convolutions and
their element-wise tail) — are warmed up, then timed ALTERNATELY with HIP events around each step, so that a drift of the machine
hits both.  Each route's `torch.cuda.max_memory_allocated` over a step, above what is allocated once the inputs exist, is recorded
too.  The kernels are also timed on their own against the bytes they must move: forward two image reads (and the mask), backward
two image reads, the mask and one gradient write — nothing is saved between them.  The merge condition is evaluated here:
the fused route's median plus both IQRs is below the torch route's median, and its peak memory is no larger.  Prints one JSON line
and, with --out, writes it to a file.

    python scripts/image_loss_cost.py --steps 50 --warmup 5 --out profiles/image_loss_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import fused_image_loss  # noqa: E402
from tests.image_loss_reference import image_loss_reference, make_image_case, mse2psnr  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12      # the MI355X's specified HBM3E rate


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
    fused, torch32 = out["fused"], out["torch32"]
    out["torch32_over_fused"] = round(torch32["ms"][0] / fused["ms"][0], 2)
    out["peak_torch32_over_fused"] = round(peak["torch32"] / max(peak["fused"], 1), 2)
    out["faster_by_more_than_both_iqrs"] = bool(fused["ms"][0] + fused["iqr_ms"] + torch32["iqr_ms"] < torch32["ms"][0])
    out["peak_no_larger"] = bool(peak["fused"] <= peak["torch32"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_cost.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    f32 = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()
    routes = {"fused": lambda p, t, m: tuple(fused_image_loss(p, t, m)), "torch32": image_loss_reference}

    # training: [2, 3, 352, 480], masked, forward + backward to the rendered image
    case = make_image_case(2, 3, 352, 480, 0.1, 1, True)
    pred, target, mask = f32(case["pred"]).requires_grad_(True), f32(case["target"]), f32(case["mask"])

    def train_step(fn):
        mse, ssim = fn(pred, target, mask)
        return torch.autograd.grad(0.8 * mse + 0.2 * (1 - ssim), [pred])[0]

    first = {name: train_step(fn) for name, fn in routes.items()}
    res["training_2x3x352x480"] = {**compare(routes, train_step, a.steps, a.warmup),
                                   "max_rel_difference_of_d_pred": float((first["fused"] - first["torch32"]).abs().max() / first["torch32"].abs().max())}

    # evaluation: [1, 3, 320, 448], no mask, forward only
    case = make_image_case(1, 3, 320, 448, 0.1, 2, False)
    e_pred, e_target = f32(case["pred"]), f32(case["target"])

    def eval_step(fn):
        with torch.no_grad():
            mse, ssim = fn(e_pred, e_target, None)
            return ssim, mse2psnr(mse)

    first = {name: eval_step(fn) for name, fn in routes.items()}
    res["evaluation_1x3x320x448"] = {**compare(routes, eval_step, a.steps, a.warmup),
                                     "difference_of_ssim": float((first["fused"][0] - first["torch32"][0]).abs())}

    # the kernels alone, at the training shape
    fwd_ms, bwd_ms, mse_only_ms = [], [], []
    for i in range(a.warmup + a.steps):
        t_f, out = timed(lambda: fused_image_loss(pred, target, mask))
        t_b, _ = timed(lambda: torch.autograd.grad(0.8 * out.mse + 0.2 * (1 - out.ssim), [pred]))
        out = fused_image_loss(pred, target, mask)
        t_m, _ = timed(lambda: torch.autograd.grad(out.mse, [pred]))
        if i >= a.warmup:
            fwd_ms.append(t_f)
            bwd_ms.append(t_b)
            mse_only_ms.append(t_m)
    image, plane = pred.numel() * 4, mask.numel() * 4
    for name, v, nbytes in (("kernel_forward", fwd_ms, 2 * image + plane), ("kernel_backward", bwd_ms, 3 * image + plane),
                            ("kernel_backward_mse_only", mse_only_ms, 3 * image + plane)):
        m = statistics.median(v)
        res[name] = {**summary(v), "bytes_to_move": int(nbytes), "GB_per_s": round(nbytes / m / 1e6, 1),
                     "share_of_hbm_rate": round(nbytes / (m * 1e-3) / HBM_BYTES_PER_S, 4),
                     "note": "HIP events around the python call: launch overhead and the small torch ops of the mix included"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
