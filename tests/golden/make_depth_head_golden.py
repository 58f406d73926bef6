#!/usr/bin/env python3
"""Generates tests/golden/depth_head_*.npz by running the REFERENCE's own depth head on seeded CPU inputs:
`DepthPredictorMonocular.forward` (encoder/epipolar/depth_predictor_monocular.py), sampled and deterministic, use_transmittance
on and off, and `EncoderEpipolar.map_pdf_to_opacity` (encoder/encoder_epipolar.py) called with a stand-in `cfg`, at exponents 1
and != 1.

Runs ONLY in the build container (needs /root/reference); nothing of the reference travels: the fixtures are plain arrays —
the projection's output (forward hook), near, far, the uniform numbers (torch.rand wrapped), the chosen index (the sampler
wrapped), the depths and the opacities.  Every case is run twice on the SAME projection output and the same uniform numbers: in
float32 (the reference as it runs) and in float64 (what the restatement is compared with; the difference of the two is the
reference's own float32 error).  The inputs obey the index-margin rule of tests/depth_head_reference.py: a seed whose case
violates it is skipped for the next one.

The import works as in make_callsite_golden.py: `jaxtyping` is stubbed, the leaf files are loaded by path, and what
encoder_epipolar.py imports beyond them (datasets, backbones, the transformer) is stubbed with empty stand-ins — only
map_pdf_to_opacity is taken from it.
"""
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

from tests.depth_head_reference import margin_violations  # noqa: E402

ENC = "ggrt.model.pixelsplat.encoder"


class _Sub:
    def __getitem__(self, item):
        return object


class _Anything:
    """stands in for every class and function that encoder_epipolar.py imports and map_pdf_to_opacity never touches"""
    def __init__(self, *a, **k):
        pass

    def __class_getitem__(cls, item):
        return cls


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def load_reference():
    jt = types.ModuleType("jaxtyping")
    for n in ("Float", "Int64", "Bool", "Shaped", "Int", "UInt8"):
        setattr(jt, n, _Sub())
    sys.modules["jaxtyping"] = jt
    sys.path.insert(0, REF)
    import ggrt.geometry.projection  # noqa: F401
    import ggrt.misc.discrete_probability_distribution  # noqa: F401
    for name in ("ggrt.model", "ggrt.model.pixelsplat", ENC, ENC + ".epipolar"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    for name in ("ggrt.dataset", "ggrt.dataset.shims", "ggrt.dataset.shims.bounds_shim", "ggrt.dataset.shims.patch_shim",
                 "ggrt.dataset.types", "ggrt.model.pixelsplat.types", ENC + ".backbone", ENC + ".common",
                 ENC + ".common.gaussian_adapter", ENC + ".encoder", ENC + ".epipolar.epipolar_transformer", ENC + ".visualization",
                 ENC + ".visualization.encoder_visualizer_epipolar_cfg"):
        sys.modules.setdefault(name, _StubModule(name))

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    base = "ggrt/model/pixelsplat/encoder/"
    load(ENC + ".epipolar.conversions", base + "epipolar/conversions.py")
    load(ENC + ".epipolar.distribution_sampler", base + "epipolar/distribution_sampler.py")
    dpm = load(ENC + ".epipolar.depth_predictor_monocular", base + "epipolar/depth_predictor_monocular.py")
    enc = load(ENC + ".encoder_epipolar", base + "encoder_epipolar.py")
    return dpm.DepthPredictorMonocular, enc.EncoderEpipolar.map_pdf_to_opacity


def run_predictor(cls, features, near, far, s, srf, spp, deterministic, transmittance, dtype, logits=None, u=None):
    """one forward of the reference's module in `dtype`; `logits` / `u` given: the projection's output and torch.rand's result
    are replaced by them (cast), so that both precisions see the same numbers"""
    torch.manual_seed(0)
    module = cls(features.shape[-1], s, srf, transmittance).to(dtype)
    seen = {}

    def hook(_m, _inp, out):
        seen["logits"] = out.detach().clone()
        return None if logits is None else logits.to(dtype)

    module.projection.register_forward_hook(hook)
    sample = module.sampler.sample

    def recording_sample(*a, **k):
        index, dens = sample(*a, **k)
        seen["index"] = index.detach().clone()
        return index, dens

    module.sampler.sample = recording_sample
    rand = torch.rand

    def recording_rand(*shape, **k):
        k.pop("dtype", None)
        r = rand(*shape, dtype=torch.float32, **k) if u is None else u
        seen["u"] = r.detach().clone()
        return r.to(dtype)

    torch.rand = recording_rand
    try:
        depth, opacity = module.forward(features.to(dtype), near.to(dtype), far.to(dtype), deterministic, spp)
    finally:
        torch.rand = rand
    seen.update(depth=depth.detach(), opacity=opacity.detach())
    return seen


class _Cfg:
    def __init__(self, initial, final, warm_up):
        self.opacity_mapping = types.SimpleNamespace(initial=initial, final=final, warm_up=warm_up)


def main():
    predictor, map_pdf_to_opacity = load_reference()
    b, v, r, d_in = 1, 2, 40, 16
    cases = [("sampled", 8, 1, 3, False, False), ("sampled_transmittance", 8, 2, 3, False, True),
             ("deterministic", 8, 1, 1, True, False), ("deterministic_transmittance", 6, 2, 2, True, True)]
    # (initial, final, warm_up, global_step) of the stand-in cfg: exponents 1, 2**0.5 and 2**-1
    mappings = [(0.0, 0.0, 1, 7), (0.5, -1.0, 100, 0), (0.5, -1.0, 100, 250)]
    for name, s, srf, spp, deterministic, transmittance in cases:
        for seed in range(100, 150):
            gen = torch.Generator().manual_seed(seed)
            features = 3.0 * torch.randn(b, v, r, d_in, generator=gen)
            near = 0.5 + torch.rand(b, v, generator=gen)
            far = 20.0 + 60.0 * torch.rand(b, v, generator=gen)
            torch.manual_seed(seed)
            f32 = run_predictor(predictor, features, near, far, s, srf, spp, deterministic, transmittance, torch.float32)
            u = f32.get("u")
            flat = f32["logits"].reshape(b * v, r, -1)
            if not bool(margin_violations(flat, srf, spp, deterministic, None if u is None else u.reshape(b * v, r, srf, spp)).any()):
                break
        else:
            raise SystemExit(f"{name}: no seed obeys the margin rule")
        f64 = run_predictor(predictor, features, near, far, s, srf, spp, deterministic, transmittance, torch.float64,
                            logits=f32["logits"], u=u)
        assert torch.equal(f32["index"], f64["index"]), name
        blob = dict(logits=f32["logits"].numpy(), near=near.numpy(), far=far.numpy(), index=f32["index"].numpy(),
                    depth32=f32["depth"].numpy(), opacity32=f32["opacity"].numpy(), depth64=f64["depth"].numpy(),
                    opacity64=f64["opacity"].numpy(), num_buckets=np.asarray(s), num_surfaces=np.asarray(srf),
                    samples=np.asarray(spp), deterministic=np.asarray(deterministic), use_transmittance=np.asarray(transmittance),
                    seed=np.asarray(seed), mapping_cfg=np.asarray(mappings, dtype=np.float64))
        if u is not None:
            blob["u"] = u.numpy()
        for i, (initial, final, warm_up, step) in enumerate(mappings):
            cfg = types.SimpleNamespace(cfg=_Cfg(initial, final, warm_up))
            blob[f"mapped32_{i}"] = map_pdf_to_opacity(cfg, f32["opacity"], step).numpy()
            blob[f"mapped64_{i}"] = map_pdf_to_opacity(cfg, f64["opacity"], step).numpy()
        path = os.path.join(OUT, f"depth_head_{name}.npz")
        np.savez_compressed(path, **blob)
        print(f"{name}: seed {seed}, index {tuple(f32['index'].shape)}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
