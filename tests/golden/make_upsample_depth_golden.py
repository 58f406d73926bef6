#!/usr/bin/env python3
"""Generates tests/golden/upsample_depth_*.npz by running the REFERENCE's own `DepthPoseNet.upsample_depth`
(ggrt/depth_pose_network.py, imported from the reference tree) and `disp_to_depth` (ggrt/geometry/depth.py) on seeded CPU inputs.
The method uses nothing of `self`, so it is called unbound, with None in its place, exactly as `DepthPoseNet.forward` calls it:
`upsample_depth(inv_depth [N,1,h,w], up_mask [N,9 r r,h,w], ratio=r, image_size=(Ho, Wo))`, then `disp_to_depth(..., 0.1, 100)[0]`.
Modules the reference imports on the way but that are not installed get stand-ins; none of them is used by the two functions.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the sizes, the upstream gradient, and for each run (float32: the reference as it runs; float64: what the restatement is
compared with) the upsampled map `out`, the gradients of sum(out * g) with respect to depth and mask, and `disp`, the map after
`disp_to_depth` (its gradients are those of `out` times the affine map's slope).  The mask is the bulk of a fixture: 9 r r logits
per cell, with their gradient in both precisions."""
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

from tests.upsample_depth_reference import INPUTS, make_upsample_case  # noqa: E402

DISP_RANGE = (0.1, 100.0)
#        name                N  h  w  r  (Ho, Wo)  seed
CASES = [("n2_r8_down_rows", 2, 3, 5, 8, (21, 40), 900),      # 24 -> 21 rows, as 384 -> 378 is a downscale; columns unchanged
         ("n1_r4_up", 1, 2, 3, 4, (13, 29), 901),              # 8 x 12 -> 13 x 29: an upscale
         ("n1_r2_one_cell", 1, 1, 1, 2, (2, 2), 902)]          # every off-centre tap is padding


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


def run(net, depth_mod, case, dtype, r, size):
    t = {k: case[k].detach().to(dtype).requires_grad_(True) for k in INPUTS}
    out = net.DepthPoseNet.upsample_depth(None, t["depth"], t["mask"], ratio=r, image_size=size)
    assert out.dtype == dtype and tuple(out.shape) == (case["depth"].shape[0], 1) + tuple(size)
    grads = torch.autograd.grad((out * case["g"].to(dtype)).sum(), [t[k] for k in INPUTS])
    disp = depth_mod.disp_to_depth(out.detach(), *DISP_RANGE)[0]
    res = dict(out=out.detach().numpy(), disp=disp.numpy())
    for k, gk in zip(INPUTS, grads):
        res["g_" + k] = gk.numpy()
    return res


def main():
    net, depth_mod = load_reference()
    for name, N, h, w, r, size, seed in CASES:
        case = {k: v.to(torch.float32) for k, v in make_upsample_case(N, h, w, r, size, seed).items()}      # the inputs ARE float32 numbers, in both runs
        blob = {k: v.numpy() for k, v in case.items()}
        blob.update(ratio=np.asarray(r), image_size=np.asarray(size), disp_range=np.asarray(DISP_RANGE), seed=np.asarray(seed))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, v in run(net, depth_mod, case, dtype, r, size).items():
                blob[k + tag] = v
        path = os.path.join(OUT, f"upsample_depth_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: mean out {blob['out64'].mean():.6f} (float32 {blob['out32'].mean():.6f}), {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
