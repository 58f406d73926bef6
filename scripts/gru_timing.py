"""What one step of the fused GRU costs beside the torch route it replaces, on one GPU.

GGRt's shape: hidden 128, input 160 (the encoder's 128 channels plus `DepthPoseNet`'s 32 of context), 48 x 63 cells; N = 1 is the
depth block, N = 5 the pose block in lock-step over five views.  One step is `SepConvGRU.forward` — the
horizontal and the vertical half-step — plus the backward to h, x and every parameter.  The two routes — `FusedSepConvGRU` (four
torch convolutions and two launches of csrc/gru_gates.hip per half-step) and the reference's forward restated literally in float32
torch on the same device (tests/gru_reference.py: two `cat`s, three convolutions and the pointwise chain per half-step) — hold the same
parameters, are warmed up, then timed ALTERNATELY with HIP events around each step, so that a drift of the machine hits both.  Each
route's device launches over one step (kernels and memsets, counted by torch's profiler in a run of its own after the timing) and
its `torch.cuda.max_memory_allocated` over a step above what is allocated once the inputs exist are recorded too.  Prints one JSON
line and, with --out, writes it to a file.

    python scripts/gru_timing.py --steps 100 --warmup 10 --out profiles/gru_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import FusedSepConvGRU  # noqa: E402
from tests.gru_reference import literal_gru, make_gru_case  # noqa: E402

DEV = "cuda:0"
CH, CX, H, W = 128, 160, 48, 63


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


def launches(step):
    """device launches of one step, by kind, from torch's profiler; a string where the profiler is not usable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not names:
            return "not measured: the profiler recorded no device event"
        ours = sum("gru_" in n and "_kernel" in n for n in names)
        copies = sum("memcpy" in n.lower() or "memset" in n.lower() for n in names)
        return {"total": len(names), "gru_gates_kernels": ours, "memcpy_memset": copies}
    except Exception as e:          # noqa: BLE001 (the count is a by-product: the timings stand without it)
        return f"not measured: {type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_timing.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "shape": {"Ch": CH, "Cx": CX, "H": H, "W": W}}
    for N in (1, 5):
        case = make_gru_case("sep", N, CH, CX, H, W, 80 + N)
        h, x, g = (case[k].to(device=DEV, dtype=torch.float32).contiguous() for k in ("h", "x", "g"))
        h.requires_grad_(True)
        x.requires_grad_(True)
        sd = {k: v.to(device=DEV, dtype=torch.float32).requires_grad_(True) for k, v in case["sd"].items()}
        fused = FusedSepConvGRU(CH, CX).to(DEV)
        fused.load_reference_state_dict({k: v.detach() for k, v in sd.items()})
        routes = {"fused": (lambda: fused(h, x), [h, x] + list(fused.parameters())),
                  "torch32": (lambda: literal_gru("sep", sd, h, x), [h, x] + list(sd.values()))}

        def step(name):
            fn, leaves = routes[name]
            out = fn()
            return (out,) + torch.autograd.grad((out * g).sum(), leaves)

        first = {name: step(name) for name in routes}
        for _ in range(a.warmup):
            for name in routes:
                step(name)
        ms, peak = {name: [] for name in routes}, {}
        for name in routes:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            step(name)
            torch.cuda.synchronize()
            peak[name] = int(torch.cuda.max_memory_allocated() - before)
        for _ in range(a.steps):
            for name in routes:
                ms[name].append(timed(lambda: step(name))[0])
        entry = {name: {**summary(v), "peak_bytes_above_inputs": peak[name]} for name, v in ms.items()}
        entry["torch32_over_fused"] = round(entry["torch32"]["ms"][0] / entry["fused"]["ms"][0], 3)
        entry["max_rel_difference"] = {k: float((p.detach() - q.detach()).abs().max() / q.detach().abs().max())
                                       for k, p, q in zip(("out", "g_h", "g_x"), first["fused"], first["torch32"])}
        fwd, bwd = {name: [] for name in routes}, {name: [] for name in routes}
        for i in range(a.warmup + a.steps):
            for name, (fn, leaves) in routes.items():
                t_f, out = timed(fn)
                t_b, _ = timed(lambda: torch.autograd.grad((out * g).sum(), leaves))
                if i >= a.warmup:
                    fwd[name].append(t_f)
                    bwd[name].append(t_b)
        for name in routes:
            entry[name]["forward"], entry[name]["backward"] = summary(fwd[name]), summary(bwd[name])
        entry["launches_per_step"] = {name: launches(lambda: step(name)) for name in routes}
        entry["bytes"] = {"one_hidden_map": N * CH * H * W * 4, "cat_buffer_the_fused_route_does_not_make": N * (CH + CX) * H * W * 4}
        res[f"n{N}_{CH}+{CX}x{H}x{W}"] = entry
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
