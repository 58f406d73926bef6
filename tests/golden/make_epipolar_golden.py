#!/usr/bin/env python3
"""Generates tests/golden/epipolar_*.npz by running the REFERENCE's own `EpipolarSampler.forward`
(encoder/epipolar/epipolar_sampler.py) and the depth lines of `EpipolarTransformer.forward` (`get_depth` of
geometry/epipolar_lines.py, the clip to [near, far], `depth_to_relative_disparity` of encoder/epipolar/conversions.py) on seeded
CPU inputs.

Runs only where the reference tree is present (`REF` below); nothing of the reference travels: the fixtures are plain arrays — the
inputs (feature maps, cameras, near, far, the sample count, the ray window) and every output, once in float32 (the reference as
it runs) and once in float64 (what the restatement is compared with; the difference of the two is the reference's own float32
error).  The inputs come from `make_case` of tests/epipolar_reference.py and so obey its margin rule.

The import works as in make_depth_head_golden.py: `jaxtyping` is stubbed and the leaf files are loaded by path.  The reference's
`sample_image_grid` returns float32 whatever the inputs are, and its float64 run fails on the mixed dtypes: the sampler's
reference to it is wrapped so that the grid is computed in the run's dtype."""
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

from tests.epipolar_reference import make_case, margin_violations  # noqa: E402

ENC = "ggrt.model.pixelsplat.encoder"
# name: (b, v, h, w, c, s, seed, family, (crop_size, clip_h, clip_w) or None).  s is a power of two: the reference computes its
# sample positions (i + 0.5) / s in float32 whatever the run's dtype, and only then are they exact in its float64 run too
CASES = {"two_views": (1, 2, 5, 7, 3, 4, 100, "default", None), "three_views": (2, 3, 4, 5, 2, 8, 200, "default", None),
         "window": (1, 2, 8, 8, 3, 4, 300, "clipped", (2, 1, 0)), "apart": (1, 2, 4, 6, 2, 4, 400, "away", None)}
OUTPUTS = ("features", "valid", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions")


class _Sub:
    def __getitem__(self, item):
        return object


def load_reference():
    jt = types.ModuleType("jaxtyping")
    for n in ("Float", "Int64", "Bool", "Shaped", "Int", "UInt8"):
        setattr(jt, n, _Sub())
    sys.modules["jaxtyping"] = jt
    sys.path.insert(0, REF)
    import ggrt.geometry.epipolar_lines as lines
    import ggrt.geometry.projection  # noqa: F401
    import ggrt.misc.heterogeneous_pairings  # noqa: F401
    for name in ("ggrt.model", "ggrt.model.pixelsplat", ENC, ENC + ".epipolar"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    base = "ggrt/model/pixelsplat/encoder/epipolar/"
    conv = load(ENC + ".epipolar.conversions", base + "conversions.py")
    sampler = load(ENC + ".epipolar.epipolar_sampler", base + "epipolar_sampler.py")
    return sampler, lines.get_depth, conv.depth_to_relative_disparity


def run(sampler_mod, get_depth, to_disparity, case, crop, dtype):
    """the reference's sampler and depth lines in `dtype`, spelled as EpipolarTransformer.forward spells them"""
    own_grid = sampler_mod.sample_image_grid

    def grid(shape, device=torch.device("cpu")):
        _, ij = own_grid(shape, device)
        axes = [(torch.arange(n, dtype=dtype) + 0.5) / n for n in reversed(shape)]      # (x coordinates, y coordinates)
        return torch.stack(torch.meshgrid(*axes, indexing="xy"), dim=-1), ij

    sampler_mod.sample_image_grid = grid
    try:
        t = lambda k: case[k].to(dtype)
        images, ext, K, near, far = t("images"), t("extrinsics"), t("intrinsics"), t("near"), t("far")
        v = images.shape[1]
        module = sampler_mod.EpipolarSampler(v, case["num_samples"])
        crop_size, clip_h, clip_w = crop if crop is not None else (None, 0, 0)
        sampling = module.forward(images, ext, K, near, far, clip_h, clip_w, crop_size)
        collect = module.collect
        b = images.shape[0]
        n_r = sampling.origins.shape[2]
        depths = get_depth(sampling.origins.reshape(b, v, 1, n_r, 1, 3), sampling.directions.reshape(b, v, 1, n_r, 1, 3),
                           sampling.xy_sample, collect(ext).reshape(b, v, v - 1, 1, 1, 4, 4), collect(K).reshape(b, v, v - 1, 1, 1, 3, 3))
        depths = depths.maximum(near[..., None, None, None])
        depths = depths.minimum(far[..., None, None, None])
        rel = to_disparity(depths, near.reshape(b, v, 1, 1, 1), far.reshape(b, v, 1, 1, 1))
    finally:
        sampler_mod.sample_image_grid = own_grid
    out = {k: getattr(sampling, k).detach() for k in OUTPUTS}
    out.update(raw_depth=depths.detach(), depth=rel.detach())
    return out


def main():
    sampler_mod, get_depth, to_disparity = load_reference()
    for name, (b, v, h, w, c, s, seed, family, crop) in CASES.items():
        window = None
        if crop is not None:
            k, ch, cw = crop
            window = (h // k * ch, h // k * (ch + 1), w // k * cw, w // k * (cw + 1))
        case = make_case(b, v, h, w, c, s, seed, family, window)
        assert margin_violations(case) == 0
        f32 = run(sampler_mod, get_depth, to_disparity, case, crop, torch.float32)
        f64 = run(sampler_mod, get_depth, to_disparity, case, crop, torch.float64)
        assert torch.equal(f32["valid"], f64["valid"]), name
        blob = {k: case[k].numpy() for k in ("images", "extrinsics", "intrinsics", "near", "far")}
        blob.update(num_samples=np.asarray(s), seed=np.asarray(case["seed"]),
                    ray_window=np.asarray(window if window is not None else (), dtype=np.int64))
        for tag, res in (("32", f32), ("64", f64)):
            for k, x in res.items():
                if k == "valid":
                    blob["valid"] = x.numpy()
                else:
                    blob[k + tag] = x.contiguous().numpy()
        path = os.path.join(OUT, f"epipolar_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: seed {case['seed']}, features {tuple(f64['features'].shape)}, valid {float(f64['valid'].double().mean()):.2f}, "
              f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
