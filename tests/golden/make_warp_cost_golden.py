#!/usr/bin/env python3
"""Generates tests/golden/warp_cost_*.npz by running the REFERENCE's own `DepthPoseNet.get_cost_each` and `depth_cost_calc`
(ggrt/depth_pose_network.py, imported from the reference tree, with its `Camera`, `inv2depth` and `Pose.from_vec`) on seeded CPU
inputs.  Both methods use nothing of `self`, so they are called unbound, with None in its place, exactly as `DepthPoseNet.forward`
calls them: `get_cost_each(pose [1,6], fmap, fmap_ref [1,C,h,w], inv2depth(inv_depth), K [1,3,3], ref_K [3,3], scale_factor)` per view,
stacked; `depth_cost_calc(inv_depth, fmap, fmaps_ref (a tuple), pose_list, K, ref_Ks, scale_factor)`.  Modules the reference imports
on the way but that are not installed get stand-ins; none of them is used by the two methods.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the scale factor, the two upstream gradients, and for each form ("none": the stack, "mean") the cost and the gradients of
sum(cost * g) with respect to fmap, fmaps_ref, inv_depth and poses, each in float32 (the reference as it runs) and in float64 (what
the restatement is compared with).  The reference casts the intrinsics with `.float()` and builds the target camera's identity pose
with `dtype=torch.float`; for the float64 run `torch.Tensor.float` is replaced by the identity and `torch.float` names float64, so
that the whole computation is float64."""
import importlib
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.environ.get("GGR_GOLDEN_OUT", HERE)
sys.path.insert(0, ROOT)

from tests.warp_cost_reference import INPUTS, LARGE_ANGLES, make_warp_case  # noqa: E402


class _AnythingMeta(type):
    def __getattr__(cls, name):          # (`models.ResNet` of a stand-in `torchvision.models`: a base class nobody instantiates here)
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


class _Anything(metaclass=_AnythingMeta):
    def __init__(self, *a, **k):
        pass


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def load_reference():
    sys.path.insert(0, REF)
    for _ in range(64):
        try:
            return importlib.import_module("ggrt.depth_pose_network"), importlib.import_module("ggrt.geometry.depth")
        except ModuleNotFoundError as e:
            if not e.name or e.name.startswith("ggrt"):
                raise
            for k in [k for k in sys.modules if k.startswith("ggrt")]:
                del sys.modules[k]
            sys.modules[e.name] = _StubModule(e.name)
    raise RuntimeError("the reference's depth_pose_network module does not import")


def run(net, depth_mod, case, dtype, scale_factor):
    to = lambda t: t.detach().to(dtype)
    V = case["fmaps_ref"].shape[0]
    real_float, real_dtype = torch.Tensor.float, torch.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self
        torch.float = torch.float64          # (Camera builds its identity pose with dtype=torch.float)
    out = {}
    # depth_cost_calc reaches get_cost_each through `self`: a stand-in that hands it the same unbound method
    this = types.SimpleNamespace(get_cost_each=lambda *a, **k: net.DepthPoseNet.get_cost_each(None, *a, **k))
    try:
        for form in ("none", "mean"):
            t = {k: to(case[k]).requires_grad_(True) for k in INPUTS}
            K, ref_Ks = to(case["K"]), to(case["ref_Ks"])
            refs = torch.split(t["fmaps_ref"], [1] * V, dim=0)
            pose_list = [t["poses"][j:j + 1] for j in range(V)]
            if form == "none":
                depth = depth_mod.inv2depth(t["inv_depth"])
                cost = torch.cat([net.DepthPoseNet.get_cost_each(None, pose_list[j], t["fmap"], refs[j], depth, K, ref_Ks[j], scale_factor)
                                  for j in range(V)], 0)
            else:
                cost = net.DepthPoseNet.depth_cost_calc(this, t["inv_depth"], t["fmap"], refs, pose_list, K, ref_Ks, scale_factor)
            assert cost.dtype == dtype and cost.shape == ((V if form == "none" else 1),) + tuple(case["fmap"].shape[1:])
            grads = torch.autograd.grad((cost * to(case["g_" + form])).sum(), [t[k] for k in INPUTS])
            out["cost_" + form] = cost.detach().numpy()
            for k, gk in zip(INPUTS, grads):
                out[f"g_{k}_{form}"] = gk.numpy()
    finally:
        torch.Tensor.float, torch.float = real_float, real_dtype
    return out


def main():
    net, depth_mod = load_reference()
    #        name           V  C  h  w   seed  scale   options
    cases = [("v2c3_eighth", 2, 3, 9, 12, 800, 1.0 / 8, {}),
             ("v3c5_unit_far", 3, 5, 6, 7, 801, 1.0, dict(partly_out=1)),
             ("v1c1_tiny", 1, 1, 2, 2, 802, 1.0 / 8, {}),
             ("v2c3_large_angles", 2, 3, 7, 10, 803, 1.0 / 8, dict(angles=LARGE_ANGLES[:2]))]
    for name, V, C, h, w, seed, scale, opts in cases:
        partly_out = opts.pop("partly_out", None)
        case = make_warp_case(V, C, h, w, seed, scale_factor=scale, **opts)
        if partly_out is not None:          # one view partly out of frame: its samples are moved by about a third of the width
            case["poses"][partly_out, 0] += 0.9
        case = {k: v.to(torch.float32) for k, v in case.items()}          # the inputs ARE float32 numbers, in both runs
        blob = {k: v.numpy() for k, v in case.items()}
        blob.update(scale_factor=np.asarray(scale), seed=np.asarray(seed))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, v in run(net, depth_mod, case, dtype, scale).items():
                blob[k + tag] = v
        path = os.path.join(OUT, f"warp_cost_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: mean cost {blob['cost_mean64'].mean():.6f} (float32 {blob['cost_mean32'].mean():.6f}), zeros in the stack "
              f"{float((blob['cost_none64'] == 0).mean()):.3f}, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
