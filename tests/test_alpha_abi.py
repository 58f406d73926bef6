"""The accumulated-opacity output (GgrForwardExtra / GgrBackwardExtra, `return_alpha`) — what needs no GPU: the settings
surface, the extra structs' layout and validation on all four entry points, and the composed torch reference the GPU tests
compare with (tests/alpha_reference.py), checked against central finite differences in float64."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib
from tests.alpha_reference import rasterize_alpha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1


def _settings_kwargs():
    e = torch.eye(4)
    return dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=e, projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False, debug=False)


def test_settings_default_is_off_and_the_shim_keeps_the_field():
    from ggrt_official_amd import GaussianRasterizationSettings
    import diff_gaussian_rasterization as dgr
    assert GaussianRasterizationSettings(**_settings_kwargs()).return_alpha is False
    assert GaussianRasterizationSettings._fields[-1] == "return_alpha"   # appended: positional construction still works
    s = dgr.GaussianRasterizationSettings(**_settings_kwargs(), return_alpha=True)
    assert s.return_alpha is True
    # the shim keeps the flag when it fills in its SH-cap default
    assert dgr.GaussianRasterizer(s)._settings_for_call().return_alpha is True


def test_decoder_output_takes_alpha_last():
    from ggrt_official_amd.splatting import DecoderOutput
    c, d = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert DecoderOutput(c, d).alpha is None                  # positional construction as before
    assert DecoderOutput(c, d, d).alpha is d


def test_extra_structs_layout_matches_header(tmp_path):
    src = tmp_path / "ext.c"
    fields = {"GgrForwardExtra": ("struct_size", "reserved", "out_alpha"),
              "GgrBackwardExtra": ("struct_size", "reserved", "dL_dout_alpha")}
    body = "".join(f'  printf("{n} %zu' + " %zu" * len(fs) + '\\n", sizeof(' + n + ")" +
                   "".join(f", offsetof({n}, {f})" for f in fs) + ");\n" for n, fs in fields.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in out:
        if not line.strip():
            continue
        name, size, *offs = line.split()
        cls = getattr(_lib, name)
        assert ctypes.sizeof(cls) == int(size) == 16, name
        assert [f for f, _ in cls._fields_] == list(fields[name]), name
        for f, off in zip(fields[name], offs):
            assert getattr(cls, f).offset == int(off), (name, f)
        seen += 1
    assert seen == 2
    assert _lib.forward_extra(1234).struct_size == 16 and _lib.forward_extra(1234).out_alpha == 1234
    assert _lib.backward_extra(5678).struct_size == 16 and _lib.backward_extra(5678).reserved == 0


def _call(which, extra):
    """One of the four entry points with `extra` and otherwise empty structs (nothing valid to render)."""
    lib = _lib.load()
    st, fin, fout = _lib.GgrSettings(), _lib.GgrForwardIn(), _lib.GgrForwardOut()
    bin_, bout, vw = _lib.GgrBackwardIn(), _lib.GgrBackwardOut(), _lib.GgrViews()
    alloc = _lib.ALLOC_FN(lambda _c, _n: None)
    ex = None if extra is None else ctypes.byref(extra)
    B = ctypes.byref
    if which == "forward":
        return lib.ggr_forward_ext(B(st), None, ex, B(fin), B(fout), alloc, None, None)
    if which == "forward_views":
        return lib.ggr_forward_views_ext(B(st), None, ex, B(vw), B(fin), B(fout), alloc, None, None)
    if which == "backward":
        return lib.ggr_backward_ext(B(st), ex, B(bin_), B(bout), None)
    return lib.ggr_backward_views_ext(B(st), ex, B(vw), B(bin_), B(bout), None)


@pytest.mark.parametrize("which", ["forward", "forward_views", "backward", "backward_views"])
@pytest.mark.parametrize("struct_size,reserved,msg", [(0, 0, "struct_size"), (8, 0, "struct_size"), (-16, 0, "struct_size"),
                                                      (16, 1, "reserved"), (16, -1, "reserved")])
def test_bad_extras_are_refused_before_any_gpu_work(which, struct_size, reserved, msg):
    cls = _lib.GgrForwardExtra if which.startswith("forward") else _lib.GgrBackwardExtra
    rc = _call(which, cls(struct_size=struct_size, reserved=reserved))
    assert rc == GGR_E_INVALID, rc
    assert msg in _lib.last_error()


@pytest.mark.parametrize("which", ["forward", "forward_views", "backward", "backward_views"])
def test_null_and_valid_extras_reach_the_next_check(which):
    """NULL extras and well-formed ones pass this check as the calls without `_ext` would: the call then ends as the plain
    entry point does (refused for the empty outputs / views; ggr_backward has no Gaussians to differentiate and returns 0)."""
    lib = _lib.load()
    cls = _lib.GgrForwardExtra if which.startswith("forward") else _lib.GgrBackwardExtra
    rc_null = _call(which, None)
    err_null = _lib.last_error()
    rc_ok = _call(which, cls(struct_size=16, reserved=0))
    err_ok = _lib.last_error()
    st, fin, fout = _lib.GgrSettings(), _lib.GgrForwardIn(), _lib.GgrForwardOut()
    bin_, bout, vw = _lib.GgrBackwardIn(), _lib.GgrBackwardOut(), _lib.GgrViews()
    alloc = _lib.ALLOC_FN(lambda _c, _n: None)
    B = ctypes.byref
    rc_plain = {"forward": lambda: lib.ggr_forward(B(st), B(fin), B(fout), alloc, None, None),
                "forward_views": lambda: lib.ggr_forward_views(B(st), B(vw), B(fin), B(fout), alloc, None, None),
                "backward": lambda: lib.ggr_backward(B(st), B(bin_), B(bout), None),
                "backward_views": lambda: lib.ggr_backward_views(B(st), B(vw), B(bin_), B(bout), None)}[which]()
    assert rc_null == rc_ok == rc_plain == (0 if which == "backward" else GGR_E_INVALID)
    assert err_null == err_ok == _lib.last_error()
    assert "struct_size" not in err_null and "reserved" not in err_null


# ---- the composed reference itself, float64 -------------------------------------------------------------------------------
def _scene64():
    """Five Gaussians in front of a 40×32 camera, overlapping, one nearly opaque (so some pixels get close to the stop)."""
    dt = torch.float64
    W, H, tanx, tany = 40, 32, 0.5, 0.4
    view = torch.eye(4, dtype=dt)
    znear, zfar = 0.01, 100.0
    P = torch.zeros(4, 4, dtype=dt)
    P[0, 0], P[1, 1] = 1 / tanx, 1 / tany
    P[2, 2], P[2, 3], P[3, 2] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
    proj = view @ P.T
    means = torch.tensor([[0.1, 0.05, 3.0], [-0.3, 0.2, 4.0], [0.4, -0.3, 5.0], [0.02, -0.02, 2.5], [0.25, 0.3, 4.5]],
                         dtype=dt)
    cov = torch.tensor([[0.02, 0.003, 0.001, 0.015, 0.002, 0.01], [0.05, -0.01, 0.0, 0.03, 0.004, 0.02],
                        [0.03, 0.0, 0.002, 0.04, -0.003, 0.03], [0.004, 0.0, 0.0, 0.003, 0.0, 0.004],
                        [0.04, 0.01, 0.0, 0.02, 0.0, 0.02]], dtype=dt)
    op = torch.tensor([[0.8], [0.6], [0.9], [0.97], [0.5]], dtype=dt)
    colors = torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.7, 0.7, 0.2], [0.3, 0.9, 0.9]], dtype=dt)
    return W, H, tanx, tany, view, proj, means, cov, op, colors


def _loss(W, H, tanx, tany, view, proj, means, cov, op, colors, g, antialiasing=False):
    _c, _r, _d, alpha = rasterize_alpha(means, op, view, proj, torch.zeros(3, dtype=torch.float64),
                                        torch.tensor([0.3, 0.6, 0.9], dtype=torch.float64), W, H, tanx, tany,
                                        colors_precomp=colors, cov3D_precomp=cov, antialiasing=antialiasing)
    return (alpha * g).sum(), alpha


def test_composed_alpha_is_one_minus_final_T():
    from oracle import torch_raster as tr
    W, H, tanx, tany, view, proj, means, cov, op, colors = _scene64()
    _, alpha = _loss(W, H, tanx, tany, view, proj, means, cov, op, colors, torch.ones(H, W, dtype=torch.float64))
    pre = tr.preprocess(means, op, view, proj, torch.zeros(3, dtype=torch.float64), W, H, tanx, tany, 0, None, colors, cov)
    pl, rg, _k, _n = tr.bin_tiles(pre, W, H)
    final_T = tr.blend(pre, pl, rg, torch.zeros(3, dtype=torch.float64), W, H)[1]
    torch.testing.assert_close(alpha.detach(), 1.0 - final_T, atol=1e-14, rtol=0)
    assert float(alpha.max()) > 0.9 and float(alpha.min()) == 0.0   # dense centre, empty corners


@pytest.mark.parametrize("which", ["means3D", "cov3D", "opacity"])
@pytest.mark.parametrize("antialiasing", [False, True])
def test_composed_reference_gradients_match_finite_differences(which, antialiasing):
    W, H, tanx, tany, view, proj, means, cov, op, colors = _scene64()
    g = torch.randn(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    leaves = dict(means3D=means.clone().requires_grad_(), cov3D=cov.clone().requires_grad_(), opacity=op.clone().requires_grad_())
    loss, _ = _loss(W, H, tanx, tany, view, proj, leaves["means3D"], leaves["cov3D"], leaves["opacity"], colors, g,
                    antialiasing)
    loss.backward()
    grad = leaves[which].grad
    base = dict(means3D=means, cov3D=cov, opacity=op)
    x = base[which]
    eps = {"means3D": 1e-6, "cov3D": 1e-9, "opacity": 1e-6}[which]
    checked = 0
    for gi in range(x.shape[0]):
        for k in range(x.shape[1]):
            xp, xm = x.clone(), x.clone()
            xp[gi, k] += eps
            xm[gi, k] -= eps
            args = dict(base)
            args[which] = xp
            lp, _ = _loss(W, H, tanx, tany, view, proj, args["means3D"], args["cov3D"], args["opacity"], colors, g,
                          antialiasing)
            args[which] = xm
            lm, _ = _loss(W, H, tanx, tany, view, proj, args["means3D"], args["cov3D"], args["opacity"], colors, g,
                          antialiasing)
            fd = float((lp - lm) / (2 * eps))
            an = float(grad[gi, k])
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 1e-4 * abs(an), (which, gi, k, fd, an)
            checked += 1
    assert checked >= 5
    assert float(grad.abs().max()) > 0.0
