"""The projection pass driven from plain C (`tests/c_abi/projection_smoke.c`, gcc, C11): the header's additions are valid C, the
library links, every invalid pass is refused before anything is enqueued, and (on the GPU) forward + ggr_projection +
ggr_projection_backward + ggr_backward give, for a tiny scene, the arrays and gradients the Python binding gives for the same
inputs.  The C host seeds an UNCLEARED scratch (scratch_zeroed = 0: the records are written), the binding adds into the scratch
its forward cleared (scratch_zeroed = 1: 0 + x): the same kernels behind both, so the figures are held to equality."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "projection_smoke.c")
LIBDIR = os.path.join(ROOT, "ggrt_official_amd")


def _build(out):
    from ggrt_official_amd import _build
    _build.build_library()
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-D__HIP_PLATFORM_AMD__", SRC,
           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-L" + LIBDIR, "-L/opt/rocm/lib", "-lggr_raster",
           "-lamdhip64", "-lm", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def test_projection_host_compiles_and_links_from_c(tmp_path):
    assert os.path.getsize(_build(str(tmp_path / "projection_smoke"))) > 0


def _python_path():
    """the scene and the gradients of projection_smoke.c through the torch binding"""
    import torch
    from ggrt_official_amd import GaussianRasterizationSettings, GaussianRasterizer
    dev = "cuda:0"
    W, H, P = 33, 17, 5
    f32 = np.float32
    tanx, tany = 1.0, f32(H) / f32(W)
    fxn, fyn, zn, zf = f32(0.5) / f32(tanx), f32(0.5) / f32(tany), f32(1), f32(100)
    proj = np.array([[2 * zn * fxn, 0, 0, 0], [0, 2 * zn * fyn, 0, 0], [0, 0, zf / (zf - zn), 1], [0, 0, -(zf * zn) / (zf - zn), 0]], f32)
    means = np.array([[0.5, 0.25, 4], [-0.25, 0.125, 2], [1.0, -0.5, 5], [0, 0, 3], [0, 0, -3]], f32)
    i = np.arange(P, dtype=f32)
    cov = np.stack([f32(0.09) + f32(0.01) * i, f32(0.01) * i, 0 * i, 0 * i + f32(0.06), f32(-0.005) * i, 0 * i + f32(0.09)], 1).astype(f32)
    k = np.arange(3, dtype=f32)
    colors = (f32(0.125) * (i[:, None] + k[None] + 1)).astype(f32)
    g = dict(means2d=np.stack([f32(0.5) - f32(0.25) * i, f32(0.125) * (i + 1)], 1), depth=f32(1.0) - f32(0.5) * i,
             conic=f32(0.25) * (k[None] - 1) + f32(0.125) * i[:, None], opacity=f32(0.75) * (i + 1), color=f32(0.5) * (i[:, None] - k[None]))
    g = {f: np.array(v, f32) for f, v in g.items()}
    for v in g.values():
        v[4] = np.nan   # the culled row
    t = lambda a: torch.tensor(np.asarray(a, f32), device=dev)
    leaf = lambda a: t(a).requires_grad_(True)
    lv = dict(means3D=leaf(means), colors_precomp=leaf(colors), opacities=leaf([0.3, 0.5, 0.9, 0.7, 0.9]), cov3D_precomp=leaf(cov))
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=float(tanx), tanfovy=float(tany), bg=t([0, 0, 0]),
                                       scale_modifier=1.0, viewmatrix=t(np.eye(4)), projmatrix=t(proj), sh_degree=0,
                                       campos=t([0, 0, 0]), prefiltered=False, return_projection=True)
    p = GaussianRasterizer(rs)(means2D=m2d, **lv)[-1]
    torch.autograd.backward([getattr(p, f) for f in g], [t(v) for v in g.values()])
    torch.cuda.synchronize()
    out = {f: getattr(p, f).detach().cpu().numpy() for f in g}
    out["valid"] = p.valid.cpu().numpy().astype(np.int64)
    out.update(dL_dmeans3D=lv["means3D"].grad, dL_dmeans2D=m2d.grad, dL_dcolors_precomp=lv["colors_precomp"].grad,
               dL_dopacities=lv["opacities"].grad, dL_dcov3D=lv["cov3D_precomp"].grad)
    return {k_: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k_, v in out.items()}


@pytest.mark.gpu
def test_c_host_projection_equals_the_python_binding(tmp_path):
    exe = _build(str(tmp_path / "projection_smoke"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "PROJECTION C ABI SMOKE OK" in r.stdout, r.stdout
    got = {}
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        if vals and name != "PROJECTION":
            got[name] = np.array([float(v) for v in vals], np.float32)
    want = _python_path()
    assert set(want) <= set(got), sorted(got)
    for name, w in want.items():
        a, b = got[name].reshape(-1), np.asarray(w).reshape(-1)
        print(name, a, b)
        assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a.astype(np.float64), b.astype(np.float64)), name
    assert want["valid"].tolist() == [1, 1, 1, 1, 0] and np.any(want["dL_dcov3D"][:4]) and not np.any(want["dL_dcov3D"][4])
