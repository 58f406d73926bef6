#!/usr/bin/env python3
"""Generates tests/golden/epi_attention_*.npz by running the REFERENCE's own `Attention.forward(x, z)`
(ggrt/model/pixelsplat/transformer/attention.py, `selfatt=False`) as `EpipolarTransformer.forward` calls it — one query token per
ray, the ray's samples as keys and values — on seeded CPU inputs.

Runs only where the reference tree is present (`REF` below); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the weights (`to_q.weight`, `to_kv.weight`, `to_out[0].weight` / `.bias`), the upstream gradient, the output and every
gradient, once in float32 (the reference as it runs) and once in float64 (what the restatement is compared with; the difference
of the two is the reference's own float32 error).  The inputs come from `make_case` of tests/epipolar_attention_reference.py.

The file is loaded by path, as in make_epipolar_golden.py; it needs torch and einops only."""
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

from tests.epipolar_attention_reference import make_case  # noqa: E402

# name: (N, S, dim, kv_dim, H, D, seed, project_out)
CASES = {"two_heads": (5, 4, 6, 6, 2, 3, 500, True), "four_heads": (3, 8, 8, 5, 4, 2, 600, True),
         "no_projection": (4, 5, 6, 4, 1, 6, 700, False)}
TENSORS = ("x", "z", "w_q", "w_kv", "w_out", "b_out")


def load_reference():
    spec = importlib.util.spec_from_file_location("ggrt_reference_attention", os.path.join(REF, "ggrt/model/pixelsplat/transformer/attention.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Attention


def run(Attention, case, dims, dtype):
    n, s, dim, kv_dim, heads, d = dims
    module = Attention(dim, heads=heads, dim_head=d, dropout=0.0, selfatt=False, kv_dim=kv_dim).to(dtype)
    project_out = case["w_out"] is not None
    assert project_out == isinstance(module.to_out, torch.nn.Sequential)
    with torch.no_grad():
        module.to_q.weight.copy_(case["w_q"])
        module.to_kv.weight.copy_(case["w_kv"])
        if project_out:
            module.to_out[0].weight.copy_(case["w_out"])
            module.to_out[0].bias.copy_(case["b_out"])
    x = case["x"].to(dtype).requires_grad_(True)
    z = case["z"].to(dtype).requires_grad_(True)
    out = module(x, z)
    leaves = {"x": x, "z": z, "w_q": module.to_q.weight, "w_kv": module.to_kv.weight}
    if project_out:
        leaves.update(w_out=module.to_out[0].weight, b_out=module.to_out[0].bias)
    grads = torch.autograd.grad(out, list(leaves.values()), case["g_out"].to(dtype))
    res = {"g_" + k: g.detach() for k, g in zip(leaves, grads)}
    res["out"] = out.detach()
    return res


def main():
    Attention = load_reference()
    for name, (n, s, dim, kv_dim, heads, d, seed, project_out) in CASES.items():
        case = make_case(n, s, dim, kv_dim, heads, d, seed, project_out)
        blob = {k: case[k].numpy() for k in TENSORS if case[k] is not None}
        blob.update(g_out=case["g_out"].numpy(), heads=np.asarray(heads), seed=np.asarray(seed))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, t in run(Attention, case, (n, s, dim, kv_dim, heads, d), dtype).items():
                blob[k + tag] = t.contiguous().numpy()
        path = os.path.join(OUT, f"epi_attention_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: seed {seed}, out {tuple(blob['out64'].shape)}, {len(blob)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
