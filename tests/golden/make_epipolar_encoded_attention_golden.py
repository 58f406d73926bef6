#!/usr/bin/env python3
"""Generates tests/golden/epi_attention_enc_*.npz by running the REFERENCE's own modules — `PositionalEncoding(O)`,
`nn.Linear(2·O, C)` behind it and `Attention(..., selfatt=False, kv_dim=C)` — composed exactly as `EpipolarTransformer.forward`
composes them (encoder/epipolar/epipolar_transformer.py lines 120-121 and 157-160):

    depths = depth_encoding(depths[..., None]);  q = sampling.features + depths;  attention(x, rearrange(q, "b v () r s c -> (b v r) s c"))

on seeded CPU inputs: one query token per ray, the ray's encoded samples as keys and values.

Runs only where the reference tree is present (`REF` below); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the weights (`depth_encoding[1].weight` / `.bias`, `to_q.weight`, `to_kv.weight`, `to_out[0].weight` / `.bias`), the
upstream gradient, the output and every gradient (x, features, depth and each weight), once in float32 (the reference as it runs)
and once with the modules `.double()` (the encoding's float32 constants widened, not recomputed: what the restatement is compared
with).  The inputs come from `make_enc_case` of tests/epipolar_encoded_attention_reference.py.

`jaxtyping` is stubbed as in make_epipolar_golden.py and the two files are loaded by path; it needs torch and einops only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from einops import rearrange

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.environ.get("GGR_GOLDEN_OUT", HERE)
sys.path.insert(0, ROOT)

from tests.epipolar_encoded_attention_reference import make_enc_case  # noqa: E402

# name: (N, S, dim, kv_dim, H, D, O, seed, project_out)
CASES = {"ten_octaves": (5, 4, 6, 6, 2, 3, 10, 510, True), "one_octave": (3, 8, 8, 5, 4, 2, 1, 610, True),
         "no_projection": (4, 5, 6, 4, 1, 6, 3, 710, False)}
TENSORS = ("x", "features", "depth", "w_enc", "b_enc", "w_q", "w_kv", "w_out", "b_out")


class _Sub:
    def __getitem__(self, item):
        return object


def load_reference():
    jt = types.ModuleType("jaxtyping")
    for n in ("Float", "Int64", "Bool", "Shaped", "Int", "UInt8"):
        setattr(jt, n, _Sub())
    sys.modules["jaxtyping"] = jt

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    return (load("ggrt_reference_positional_encoding", "ggrt/model/pixelsplat/encodings/positional_encoding.py").PositionalEncoding,
            load("ggrt_reference_attention", "ggrt/model/pixelsplat/transformer/attention.py").Attention)


def run(PositionalEncoding, Attention, case, dims, dtype):
    n, s, dim, kv_dim, heads, d, octaves = dims
    pe = PositionalEncoding(octaves)
    depth_encoding = torch.nn.Sequential(pe, torch.nn.Linear(pe.d_out(1), kv_dim)).to(dtype)
    attention = Attention(dim, heads=heads, dim_head=d, dropout=0.0, selfatt=False, kv_dim=kv_dim).to(dtype)
    project_out = case["w_out"] is not None
    assert project_out == isinstance(attention.to_out, torch.nn.Sequential)
    with torch.no_grad():
        depth_encoding[1].weight.copy_(case["w_enc"])
        depth_encoding[1].bias.copy_(case["b_enc"])
        attention.to_q.weight.copy_(case["w_q"])
        attention.to_kv.weight.copy_(case["w_kv"])
        if project_out:
            attention.to_out[0].weight.copy_(case["w_out"])
            attention.to_out[0].bias.copy_(case["b_out"])
    x = case["x"].to(dtype).requires_grad_(True)
    features = case["features"].to(dtype).requires_grad_(True)
    depth = case["depth"].to(dtype).requires_grad_(True)
    # the sampler's layout, one batch, one view, one other view: features [b,v,ov,r,s,c] and depths [b,v,ov,r,s]
    depths = depth_encoding(depth.reshape(1, 1, 1, n, s)[..., None])
    q = features.reshape(1, 1, 1, n, s, kv_dim) + depths
    out = attention(x, rearrange(q, "b v () r s c -> (b v r) s c"))
    leaves = {"x": x, "features": features, "depth": depth, "w_enc": depth_encoding[1].weight, "b_enc": depth_encoding[1].bias,
              "w_q": attention.to_q.weight, "w_kv": attention.to_kv.weight}
    if project_out:
        leaves.update(w_out=attention.to_out[0].weight, b_out=attention.to_out[0].bias)
    grads = torch.autograd.grad(out, list(leaves.values()), case["g_out"].to(dtype))
    res = {"g_" + k: g.detach() for k, g in zip(leaves, grads)}
    res["out"] = out.detach()
    return res


def main():
    PositionalEncoding, Attention = load_reference()
    for name, (n, s, dim, kv_dim, heads, d, octaves, seed, project_out) in CASES.items():
        case = make_enc_case(n, s, dim, kv_dim, heads, d, octaves, seed, project_out)
        blob = {k: case[k].numpy() for k in TENSORS if case[k] is not None}
        blob.update(g_out=case["g_out"].numpy(), heads=np.asarray(heads), num_octaves=np.asarray(octaves), seed=np.asarray(seed))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, t in run(PositionalEncoding, Attention, case, (n, s, dim, kv_dim, heads, d, octaves), dtype).items():
                blob[k + tag] = t.contiguous().numpy()
        path = os.path.join(OUT, f"epi_attention_enc_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: seed {seed}, out {tuple(blob['out64'].shape)}, {len(blob)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
