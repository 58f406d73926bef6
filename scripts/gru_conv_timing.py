"""What one inference step of the GRU costs on each of its three routes, on one GPU.

GGRt's shape: hidden 128, input 160, 48 x 63 cells; N = 1 is the depth block, N = 5 the pose block in lock-step over five views.
One step is `SepConvGRU.forward` — the horizontal and the vertical half-step — under `torch.no_grad()`, parameters frozen.  Three
routes hold the same parameters, are warmed up, then timed ALTERNATELY in one process with HIP events around each step, so that a
drift of the machine hits all three:

    hip_convs   `FusedSepConvGRU(hip_convs=True)`: two launches of csrc/gru_conv.hip per half-step, convolutions included
    parent      `FusedSepConvGRU()`: four torch convolutions and two launches of csrc/gru_gates.hip per half-step — the code before
                the flag existed, byte for byte, and therefore the baseline
    torch32     the reference's forward restated literally in float32 torch (`run_gru("literal", ...)`, tests/gru_reference.py)

Beside the medians (with min, max and the interquartile range) it records the half-step's algorithmic FLOPs — 2 (Ch + Cx) taps x 3 Ch
per pixel, two half-steps per step — the rate the hip_convs route reaches on them as an END-TO-END figure (event time of the whole
step, launches and the two pointwise tails included, not a kernel's time), and its share of the 155 TFLOP/s that the float32 MFMA
reaches on this part.  Prints one JSON line and, with --out, writes it to a file.

    python scripts/gru_conv_timing.py --steps 200 --warmup 20 --out profiles/gru_conv_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggrt_official_amd import FusedSepConvGRU  # noqa: E402
from tests.gru_reference import literal_gru, make_gru_case, run_gru  # noqa: E402

DEV = "cuda:0"
CH, CX, H, W, TAPS = 128, 160, 48, 63, 5
F32_MFMA_PEAK_TFLOPS = 155.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_conv_timing.py measures on the GPU: none found")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "shape": {"Ch": CH, "Cx": CX, "H": H, "W": W},
           "f32_mfma_peak_tflops": F32_MFMA_PEAK_TFLOPS}
    with torch.no_grad():
        for N in (1, 5):
            case = make_gru_case("sep", N, CH, CX, H, W, 90 + N)
            h, x = (case[k].to(device=DEV, dtype=torch.float32).contiguous() for k in ("h", "x"))
            sd = {k: v.to(device=DEV, dtype=torch.float32) for k, v in case["sd"].items()}
            modules = {}
            for name, flag in (("hip_convs", True), ("parent", False)):
                modules[name] = FusedSepConvGRU(CH, CX, hip_convs=flag).to(DEV).requires_grad_(False)
                modules[name].load_reference_state_dict(sd)
            # (run_gru("literal", ...) copies the case to the device on every call: its forward, `literal_gru`, is timed on prepared
            # tensors, and one run_gru call is compared with it below)
            routes = {"hip_convs": lambda: modules["hip_convs"](h, x), "parent": lambda: modules["parent"](h, x),
                      "torch32": lambda: literal_gru("sep", sd, h, x)}
            first = {name: fn() for name, fn in routes.items()}
            first["run_gru"] = run_gru("literal", "sep", case, torch.float32, DEV, need=())["out"]
            for _ in range(a.warmup):
                for fn in routes.values():
                    fn()
            ms = {name: [] for name in routes}
            for _ in range(a.steps):
                for name, fn in routes.items():
                    ms[name].append(timed(fn)[0])
            entry = {name: summary(v) for name, v in ms.items()}
            med = {name: entry[name]["ms"][0] for name in routes}
            entry["parent_over_hip_convs"] = round(med["parent"] / med["hip_convs"], 3)
            entry["torch32_over_hip_convs"] = round(med["torch32"] / med["hip_convs"], 3)
            flop = 2 * 2.0 * (CH + CX) * TAPS * 3 * CH * N * H * W          # two half-steps
            tflops = flop / (med["hip_convs"] * 1e-3) / 1e12
            entry["flop_per_step"] = flop
            entry["hip_convs_end_to_end_tflops"] = round(tflops, 2)
            entry["hip_convs_share_of_f32_mfma_peak"] = round(tflops / F32_MFMA_PEAK_TFLOPS, 4)
            entry["least_ms_at_peak"] = round(flop / (F32_MFMA_PEAK_TFLOPS * 1e12) * 1e3, 4)
            ref = first["torch32"]
            entry["max_rel_difference_to_torch32"] = {k: float((first[k] - ref).abs().max() / ref.abs().max()) for k in ("hip_convs", "parent", "run_gru")}
            res[f"n{N}_{CH}+{CX}x{H}x{W}"] = entry
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
