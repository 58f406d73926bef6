#!/usr/bin/env python3
"""Generates tests/golden/photometric_loss_*.npz by running the REFERENCE's own `MultiViewPhotometricDecayLoss`
(ggrt/loss/photometric_loss.py, imported from the reference tree, with its `Camera`, `inv2depth`, `calc_smoothness` and
`Pose.from_vec`) on seeded CPU inputs.  Modules the reference imports on the way but that are not installed get stand-ins; none of
them is used by the loss.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the settings, and the loss, both metrics and both gradients, each in float32 (the reference as it runs) and in float64 (what
the restatement is compared with).  One accommodation for the CPU: the reference moves its cameras with
`.to(ref_image.get_device())`, which is -1 on the CPU and not a device; `Camera.to` is replaced by a no-op for the run.  The
reference casts the intrinsics with `.float()`; for the float64 run `torch.Tensor.float` is replaced by the identity and
`torch.float` names float64, so that the whole computation is float64."""
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

from tests.photometric_loss_reference import make_photometric_case  # noqa: E402


class _Anything:
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
    for _ in range(32):
        try:
            mod = importlib.import_module("ggrt.loss.photometric_loss")
            break
        except ModuleNotFoundError as e:
            if not e.name or e.name.startswith("ggrt.loss"):
                raise
            for k in [k for k in sys.modules if k.startswith("ggrt")]:
                del sys.modules[k]
            sys.modules[e.name] = _StubModule(e.name)
    else:
        raise RuntimeError("the reference's loss module does not import")
    camera = importlib.import_module("ggrt.geometry.camera")
    camera.Camera.to = lambda self, *a, **k: self
    return mod


def run(mod, case, dtype, opts):
    to = lambda t: t.detach().to(dtype)
    inv = [to(d)[None].requires_grad_(True) for d in case["inv_depths"]]          # n x [1,1,H,W], as the reference receives them
    poses = to(case["poses"]).requires_grad_(True)
    loss_fn = mod.MultiViewPhotometricDecayLoss(**opts)
    real_float, real_dtype = torch.Tensor.float, torch.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self
        torch.float = torch.float64          # (Camera builds its identity pose with dtype=torch.float)
    try:
        out = loss_fn(to(case["image"]), to(case["ref_imgs"]), inv, to(case["K"]), to(case["ref_Ks"]), poses)
    finally:
        torch.Tensor.float, torch.float = real_float, real_dtype
    assert out["loss"].dtype == dtype and out["loss"].shape == (1,)
    grads = torch.autograd.grad(out["loss"].sum(), inv + [poses])
    zero = torch.zeros((), dtype=dtype)
    return dict(loss=out["loss"].detach().numpy(), photometric_loss=out["metrics"]["photometric_loss"].numpy(),
                smoothness_loss=out["metrics"].get("smoothness_loss", zero).numpy(),
                g_inv_depths=torch.cat(grads[:-1], 0).numpy(), g_poses=grads[-1].numpy())


def main():
    mod = load_reference()
    #        name            V  n  H   W  seed  options
    cases = [("v2n3_default", 2, 3, 17, 24, 700, {}),
             ("v3n2_noclip_nomask", 3, 2, 24, 32, 701, dict(clip_loss=0.0, automask_loss=False, smooth_loss_weight=0.05)),
             ("v1n1_tiny", 1, 1, 5, 7, 702, dict(ssim_loss_weight=0.5, smooth_loss_weight=0.0, clip_loss=1.0))]
    for name, V, n, H, W, seed, opts in cases:
        case = make_photometric_case(V, n, H, W, seed)
        case = {k: v.to(torch.float32) for k, v in case.items()}          # the inputs ARE float32 numbers, in both runs
        blob = {k: v.numpy() for k, v in case.items()}
        blob.update(V=np.asarray(V), n=np.asarray(n), seed=np.asarray(seed))
        for k, v in opts.items():
            blob["opt_" + k] = np.asarray(v)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, v in run(mod, case, dtype, opts).items():
                blob[k + tag] = v
        path = os.path.join(OUT, f"photometric_loss_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: loss {blob['loss64']} (float32 {blob['loss32']}), photometric {blob['photometric_loss64']}, smoothness "
              f"{blob['smoothness_loss64']}, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
