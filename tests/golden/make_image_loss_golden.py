#!/usr/bin/env python3
"""Generates tests/golden/image_loss_*.npz by running the REFERENCE's own `ssim` (ggrt/loss/ssim_torch.py, loaded by path) and
`img2mse` (utils_loc.py, loaded by path with stand-ins for `cv2` / `matplotlib` where they are not installed) on seeded CPU inputs.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: the fixtures are plain arrays — the
inputs, the mask, the upstream gradients, both results and the gradients with respect to both images, each in float32 (the
reference as it runs) and in float64 (what the restatement is compared with), and the reference's 1-D window.  With
`size_average=False` the reference's `ssim` returns one value per image; `img2mse` has no such switch, so it is called once per
image with that image's mask slice."""
import importlib.util
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

from tests.image_loss_reference import make_image_case  # noqa: E402


class _Anything:
    def __init__(self, *a, **k):
        pass


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("cv2", "matplotlib", "matplotlib.backends", "matplotlib.backends.backend_agg", "matplotlib.figure"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _StubModule(name)
    return _load("ref_ssim_torch", "ggrt/loss/ssim_torch.py"), _load("ref_utils_loc", "utils_loc.py")


def run(ssim_mod, utils, case, window_size, size_average, dtype):
    to = lambda t: None if t is None else t.detach().to(dtype)
    pred, target, mask = to(case["pred"]).requires_grad_(True), to(case["target"]).requires_grad_(True), to(case["mask"])
    ssim = ssim_mod.ssim(pred, target, window_size, size_average)
    x, y = pred.permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)
    if size_average:
        mse = utils.img2mse(x, y, mask)
    else:
        mse = torch.stack([utils.img2mse(x[b], y[b], None if mask is None else mask[b]) for b in range(pred.shape[0])])
    n = mse.numel()
    loss = (mse.reshape(-1) * to(case["g_mse"])[:n]).sum() + (ssim.reshape(-1) * to(case["g_ssim"])[:n]).sum()
    d_pred, d_target = torch.autograd.grad(loss, [pred, target])
    return dict(mse=mse.detach().numpy(), ssim=ssim.detach().numpy(), d_pred=d_pred.numpy(), d_target=d_target.numpy())


def main():
    ssim_mod, utils = load_reference()
    #        name               b  c  h   w   noise seed masked window size_average
    cases = [("b2c3_masked", 2, 3, 13, 9, 0.1, 900, True, 11, True),
             ("b1c1_tiny", 1, 1, 7, 5, 0.3, 901, False, 11, True),
             ("b1c4_window7", 1, 4, 24, 17, 0.02, 902, False, 7, True),
             ("b3c3_per_image", 3, 3, 12, 14, 0.1, 903, True, 11, False)]
    for name, b, c, h, w, noise, seed, masked, window_size, size_average in cases:
        case = make_image_case(b, c, h, w, noise, seed, masked)
        blob = dict(pred=case["pred"].numpy().astype(np.float32), target=case["target"].numpy().astype(np.float32),
                    g_mse=case["g_mse"].numpy().astype(np.float32), g_ssim=case["g_ssim"].numpy().astype(np.float32),
                    window_size=np.asarray(window_size), size_average=np.asarray(size_average), noise=np.asarray(noise), seed=np.asarray(seed),
                    window=ssim_mod.gaussian(window_size, 1.5).numpy())
        if masked:
            blob["mask"] = case["mask"].numpy().astype(np.float32)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, v in run(ssim_mod, utils, case, window_size, size_average, dtype).items():
                blob[k + tag] = v
        path = os.path.join(OUT, f"image_loss_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: mse {blob['mse64']}, ssim {blob['ssim64']}, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
