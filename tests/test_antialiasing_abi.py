"""Anti-aliased rasterization (upstream's `antialiasing` setting) — what needs no GPU: the settings surface, the C ABI's
options struct and its validation, and the composed torch reference the GPU tests compare with (tests/aa_reference.py),
checked against central finite differences in float64."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib
from tests.aa_reference import AA_MIN_RATIO, aa_scale, rasterize_aa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings_kwargs():
    e = torch.eye(4)
    return dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=e, projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False, debug=False)


def test_settings_take_upstreams_antialiasing_keyword():
    from ggrt_official_amd import GaussianRasterizationSettings
    import diff_gaussian_rasterization as dgr
    s = GaussianRasterizationSettings(**_settings_kwargs(), antialiasing=True)
    assert s.antialiasing is True
    assert GaussianRasterizationSettings(**_settings_kwargs()).antialiasing is False
    s2 = dgr.GaussianRasterizationSettings(**_settings_kwargs(), antialiasing=True)
    assert s2.antialiasing is True
    # the shim keeps the flag when it fills in its SH-cap default
    assert dgr.GaussianRasterizer(s2)._settings_for_call().antialiasing is True


def test_forward_options_layout_matches_header(tmp_path):
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(GgrForwardOptions), offsetof(GgrForwardOptions, struct_size),'
                   ' offsetof(GgrForwardOptions, antialiasing));\n  return 0;\n}\n')
    exe = tmp_path / "opt"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off0, off1 = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    cls = _lib.GgrForwardOptions
    assert ctypes.sizeof(cls) == size
    assert cls.struct_size.offset == off0 and cls.antialiasing.offset == off1
    assert [f for f, _ in cls._fields_] == ["struct_size", "antialiasing"]
    assert _lib.forward_options(True).struct_size == size and _lib.forward_options(True).antialiasing == 1


@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("struct_size,aa,msg", [(4, 0, "struct_size"), (0, 1, "struct_size"), (8, 2, "antialiasing"),
                                                (8, -1, "antialiasing")])
def test_bad_options_are_refused_before_any_gpu_work(views, struct_size, aa, msg):
    lib = _lib.load()
    opt = _lib.GgrForwardOptions(struct_size=struct_size, antialiasing=aa)
    st, fin, fout = _lib.GgrSettings(), _lib.GgrForwardIn(), _lib.GgrForwardOut()
    alloc = _lib.ALLOC_FN(lambda _c, _n: None)
    if views:
        rc = lib.ggr_forward_views_opt(ctypes.byref(st), ctypes.byref(opt), ctypes.byref(_lib.GgrViews()), ctypes.byref(fin),
                                       ctypes.byref(fout), alloc, None, None)
    else:
        rc = lib.ggr_forward_opt(ctypes.byref(st), ctypes.byref(opt), ctypes.byref(fin), ctypes.byref(fout), alloc, None, None)
    assert rc == 1, rc   # GGR_E_INVALID
    assert msg in _lib.last_error()


def test_null_options_are_the_plain_forward():
    """NULL options pass validation as ggr_forward would: the next check (null outputs) is what refuses this call."""
    lib = _lib.load()
    st, fin, fout = _lib.GgrSettings(), _lib.GgrForwardIn(), _lib.GgrForwardOut()
    alloc = _lib.ALLOC_FN(lambda _c, _n: None)
    rc_opt = lib.ggr_forward_opt(ctypes.byref(st), None, ctypes.byref(fin), ctypes.byref(fout), alloc, None, None)
    err_opt = _lib.last_error()
    rc = lib.ggr_forward(ctypes.byref(st), ctypes.byref(fin), ctypes.byref(fout), alloc, None, None)
    assert rc_opt == rc == 1 and err_opt == _lib.last_error() and "null output" in err_opt


# ---- the composed reference itself, float64 -------------------------------------------------------------------------------
def _scene64():
    """Six Gaussians in front of a 40×32 camera: ordinary ones, a sub-pixel one (s well below 1) and one so thin that
    det(Σ2D)/det(Σ2D + 0.3·I) falls under the clamp."""
    dt = torch.float64
    W, H, tanx, tany = 40, 32, 0.5, 0.4
    view = torch.eye(4, dtype=dt)
    znear, zfar = 0.01, 100.0
    P = torch.zeros(4, 4, dtype=dt)
    P[0, 0], P[1, 1] = 1 / tanx, 1 / tany
    P[2, 2], P[2, 3], P[3, 2] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
    proj = view @ P.T
    means = torch.tensor([[0.1, 0.05, 3.0], [-0.3, 0.2, 4.0], [0.4, -0.3, 5.0], [0.02, -0.02, 2.5],
                          [-0.2, -0.25, 3.5], [0.25, 0.3, 4.5]], dtype=dt)
    cov = torch.tensor([[0.02, 0.003, 0.001, 0.015, 0.002, 0.01], [0.05, -0.01, 0.0, 0.03, 0.004, 0.02],
                        [0.03, 0.0, 0.002, 0.04, -0.003, 0.03], [1e-5, 2e-6, 0.0, 8e-6, 0.0, 1e-5],
                        [1e-11, 0.0, 0.0, 1e-11, 0.0, 1e-11], [0.04, 0.01, 0.0, 0.02, 0.0, 0.02]], dtype=dt)
    op = torch.tensor([[0.8], [0.6], [0.9], [0.95], [1.0], [0.5]], dtype=dt)
    colors = torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.7, 0.7, 0.2], [0.5, 0.1, 0.6],
                           [0.3, 0.9, 0.9]], dtype=dt)
    return W, H, tanx, tany, view, proj, means, cov, op, colors


def _loss(W, H, tanx, tany, view, proj, means, cov, op, colors, dL):
    color, _r, _d, pre = rasterize_aa(means, op, view, proj, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                                      W, H, tanx, tany, colors_precomp=colors, cov3D_precomp=cov)
    return (color * dL).sum(), pre


def test_composed_reference_has_sub_pixel_and_clamped_gaussians():
    W, H, tanx, tany, view, proj, means, cov, op, colors = _scene64()
    dL = torch.randn(3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    _, pre = _loss(W, H, tanx, tany, view, proj, means, cov, op, colors, dL)
    s = pre["aa_scale"]
    assert bool(pre["visible"].all())
    assert float(s[:3].min()) > 0.5 and float(s[3]) < 0.5           # sub-pixel: s ≪ 1
    assert abs(float(s[4]) - AA_MIN_RATIO ** 0.5) < 1e-12           # clamped
    torch.testing.assert_close(pre["opacity"], op.reshape(-1) * s)


@pytest.mark.parametrize("which", ["means3D", "cov3D", "opacity"])
def test_composed_reference_gradients_match_finite_differences(which):
    W, H, tanx, tany, view, proj, means, cov, op, colors = _scene64()
    dL = torch.randn(3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    leaves = dict(means3D=means.clone().requires_grad_(), cov3D=cov.clone().requires_grad_(), opacity=op.clone().requires_grad_())
    loss, _ = _loss(W, H, tanx, tany, view, proj, leaves["means3D"], leaves["cov3D"], leaves["opacity"], colors, dL)
    loss.backward()
    g = leaves[which].grad
    base = dict(means3D=means, cov3D=cov, opacity=op)
    x = base[which]
    eps = {"means3D": 1e-6, "cov3D": 1e-9, "opacity": 1e-6}[which]
    checked = 0
    for gi in range(x.shape[0]):
        for k in range(x.shape[1]):
            if which == "cov3D" and gi == 4:
                continue   # (the clamp-regime Gaussian's covariance is 1e-11: a step of 1e-9 leaves its regime)
            xp, xm = x.clone(), x.clone()
            xp[gi, k] += eps
            xm[gi, k] -= eps
            args = dict(base)
            args[which] = xp
            lp, _ = _loss(W, H, tanx, tany, view, proj, args["means3D"], args["cov3D"], args["opacity"], colors, dL)
            args[which] = xm
            lm, _ = _loss(W, H, tanx, tany, view, proj, args["means3D"], args["cov3D"], args["opacity"], colors, dL)
            fd = float((lp - lm) / (2 * eps))
            an = float(g[gi, k])
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 1e-4 * abs(an), (which, gi, k, fd, an)
            checked += 1
    assert checked >= 6


def test_aa_scale_clamp_has_no_covariance_gradient():
    conic = torch.tensor([[1 / 0.3000001, 0.0, 1 / 0.3000001]], dtype=torch.float64, requires_grad=True)
    s = aa_scale(conic)
    s.sum().backward()
    assert float(s.detach()) == pytest.approx(AA_MIN_RATIO ** 0.5) and float(conic.grad.abs().max()) == 0.0
