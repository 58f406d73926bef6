#!/usr/bin/env python3
"""Generates tests/golden/gru_*.npz by running the REFERENCE's own `SepConvGRU` and `ConvGRU` (ggrt/optimizer.py, loaded from the
reference tree by file: the module imports torch only) in float64 on the CPU, on the seeded inputs of tests/gru_reference.py:
`module.load_state_dict(sd)`, `module(h, x)`, and the gradients of sum(h' * g) with respect to h, x and every parameter.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: a fixture is plain arrays — the state
dict under the reference's keys (`sd.convz1.weight` ...), `h`, `x`, the upstream gradient `g`, the output `out`, `g_h`, `g_x` and
`g_sd.<key>` for every parameter."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.environ.get("GGR_GOLDEN_OUT", HERE)
sys.path.insert(0, ROOT)

from tests.gru_reference import make_gru_case, reference_keys  # noqa: E402

#        name        N  Ch Cx H  W  seed
CASES = [("n2_c4", 2, 4, 6, 5, 7, 1000),
         ("n1_c3", 1, 3, 2, 3, 5, 1001)]
CLASSES = {"sep": "SepConvGRU", "conv": "ConvGRU"}


def load_reference():
    spec = importlib.util.spec_from_file_location("ggrt_reference_optimizer", os.path.join(REF, "ggrt", "optimizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    for name, N, ch, cx, H, W, seed in CASES:
        for kind, cls in CLASSES.items():
            case = make_gru_case(kind, N, ch, cx, H, W, seed)
            module = getattr(ref, cls)(hidden_dim=ch, input_dim=cx).double()
            assert sorted(module.state_dict()) == sorted(reference_keys(kind))
            module.load_state_dict(case["sd"])
            h, x = case["h"].clone().requires_grad_(True), case["x"].clone().requires_grad_(True)
            out = module(h, x)
            assert out.dtype == torch.float64 and out.shape == h.shape
            (out * case["g"]).sum().backward()
            blob = dict(h=case["h"].numpy(), x=case["x"].numpy(), g=case["g"].numpy(), out=out.detach().numpy(), g_h=h.grad.numpy(), g_x=x.grad.numpy(),
                        seed=np.asarray(seed))
            params = dict(module.named_parameters())
            for k in reference_keys(kind):
                assert torch.equal(params[k].detach(), case["sd"][k])
                blob["sd." + k], blob["g_sd." + k] = case["sd"][k].numpy(), params[k].grad.numpy()
            path = os.path.join(OUT, f"gru_{kind}_{name}.npz")
            np.savez_compressed(path, **blob)
            print(f"{kind}_{name}: mean |out| {np.abs(blob['out']).mean():.6f}, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
