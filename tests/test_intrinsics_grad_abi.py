"""The intrinsics gradient (GgrBackwardExtra2.dL_dtanfov, ggr_camera_setup_backward, a differentiable `camera_setup`) — what
needs no GPU: the header and the ctypes mirror agree, a GgrBackwardExtra of the old size is still taken, dL_dtanfov without
the camera gradient outputs is refused before anything is enqueued, the float64 camera reference (tests/camera_reference.py)
reproduces the call site's torch branch, and the torch oracle differentiates tan(fov/2) given as tensors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from ggrt_official_amd import _lib
from ggrt_official_amd import splatting as sp
from tests import camera_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1


def test_extra2_layout_matches_header_and_extra_keeps_its_size(tmp_path):
    fields = ("struct_size", "reserved", "dL_dout_alpha", "dL_dtanfov")
    src = tmp_path / "ext2.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu %zu' + " %zu" * len(fields) + '\\n", sizeof(GgrBackwardExtra), sizeof(GgrBackwardExtra2)' +
                   "".join(f", offsetof(GgrBackwardExtra2, {f})" for f in fields) + ");\n"
                   '  printf("%zu %zu\\n", offsetof(GgrBackwardExtra, dL_dout_alpha), sizeof(GgrBackwardOut));\n'
                   '  printf("%d\\n", GGR_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "ext2"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    l0, l1, l2 = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:3]
    old, new, *offs = (int(x) for x in l0.split())
    assert old == ctypes.sizeof(_lib.GgrBackwardExtra) == 16          # the ABI-11 struct did not grow …
    assert new == ctypes.sizeof(_lib.GgrBackwardExtra2) == 24
    assert [f for f, _ in _lib.GgrBackwardExtra2._fields_] == list(fields)
    for f, off in zip(fields, offs):
        assert getattr(_lib.GgrBackwardExtra2, f).offset == off, f
    # … and is a prefix of the new one, field for field
    for f, _ in _lib.GgrBackwardExtra._fields_:
        assert getattr(_lib.GgrBackwardExtra, f).offset == getattr(_lib.GgrBackwardExtra2, f).offset
    alpha_off, out_size = (int(x) for x in l1.split())
    assert alpha_off == _lib.GgrBackwardExtra2.dL_dout_alpha.offset
    assert out_size == ctypes.sizeof(_lib.GgrBackwardOut) == 13 * 8   # GgrBackwardOut did not grow
    assert int(l2) == _lib.ABI_VERSION == 11
    ptr, ex = _lib.backward_extra2(1234, 5678)
    assert ex.struct_size == 24 and ex.reserved == 0 and ex.dL_dout_alpha == 1234 and ex.dL_dtanfov == 5678
    assert ptr.contents.struct_size == 24 and ptr.contents.dL_dout_alpha == 1234


def test_camera_setup_backward_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "ggr_raster.h")).read()
    assert "int ggr_camera_setup_backward(" in text
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert "ggr_camera_setup_backward" in bound and len(bound["ggr_camera_setup_backward"][1]) == 13
    lib = _lib.load()
    # bad arguments are refused before anything is enqueued
    assert lib.ggr_camera_setup_backward(2, *([None] * 4), 1, *([None] * 6), None) == GGR_E_INVALID and _lib.last_error()
    assert lib.ggr_camera_setup_backward(-1, *([None] * 4), 1, *([None] * 6), None) == GGR_E_INVALID


def _backward(which, extra, pose=False):
    """ggr_backward_ext / ggr_backward_views_ext with `extra` over empty structs: zero Gaussians, nothing reaches a GPU.
    `pose`: the three camera gradient outputs are given (never written: the call is refused first, or not made)."""
    lib = _lib.load()
    st, bin_, bout = _lib.GgrSettings(), _lib.GgrBackwardIn(), _lib.GgrBackwardOut()
    if pose:
        bout.dL_dviewmatrix, bout.dL_dprojmatrix, bout.dL_dcampos = 64, 128, 192
    B = ctypes.byref
    if which == "backward":
        return lib.ggr_backward_ext(B(st), extra, B(bin_), B(bout), None)
    vw = _lib.GgrViews(num_views=2, viewmatrix=64, projmatrix=64, campos=64, bg=64, tanfov=64)   # (never dereferenced)
    return lib.ggr_backward_views_ext(B(st), extra, B(vw), B(bin_), B(bout), None)


@pytest.mark.parametrize("which", ["backward", "backward_views"])
def test_old_size_extra_is_still_accepted_and_means_field_absent(which):
    plain = _backward(which, None)
    assert plain == 0, _lib.last_error()
    assert _backward(which, ctypes.byref(_lib.backward_extra())) == 0             # the 16-byte struct, as before
    # a GgrBackwardExtra2 whose struct_size stops at the old struct's end: the field behind it is not read
    ptr, ex = _lib.backward_extra2(None, 0xdead0)
    ex.struct_size = 16
    assert _backward(which, ptr) == 0, _lib.last_error()
    ex.struct_size = 20                                                             # (ends inside the field: absent too)
    assert _backward(which, ptr) == 0, _lib.last_error()
    # the whole struct with a NULL field: nothing requested
    ptr, ex = _lib.backward_extra2(None, None)
    assert _backward(which, ptr) == 0, _lib.last_error()


@pytest.mark.parametrize("which", ["backward", "backward_views"])
def test_dtanfov_without_the_pose_outputs_is_refused(which):
    ptr, ex = _lib.backward_extra2(None, 0xdead0)
    assert _backward(which, ptr) == GGR_E_INVALID
    assert "dL_dtanfov" in _lib.last_error() and "dL_dviewmatrix" in _lib.last_error()
    # the old checks still come first
    ex.reserved = 1
    assert _backward(which, ptr) == GGR_E_INVALID and "reserved" in _lib.last_error()
    ex.reserved, ex.struct_size = 0, 8
    assert _backward(which, ptr) == GGR_E_INVALID and "struct_size" in _lib.last_error()


def test_settings_tanfov_is_documented_as_differentiable_and_host_floats_are_not():
    from ggrt_official_amd import GaussianRasterizationSettings
    e = torch.eye(4)
    rs = GaussianRasterizationSettings(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=e, projmatrix=e, sh_degree=3, campos=torch.zeros(3),
                                       prefiltered=False, debug=False)
    assert rs.tanfov is None and isinstance(rs.tanfovx, float)
    import inspect
    from ggrt_official_amd import rasterizer
    sig = inspect.signature(rasterizer._RasterizeGaussians.forward)
    assert list(sig.parameters)[-1] == "tanfov" and sig.parameters["tanfov"].default is None


# ---- the float64 camera reference against the call site's torch branch -------------------------------------------------------
@pytest.mark.parametrize("scale_invariant", [True, False])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_camera_reference_reproduces_the_torch_branch(n, scale_invariant):
    ext, intr, near, far = cr.cameras(n, seed=n)
    # splatting.render_views_fused, the branch for CPU tensors, in float32
    e = ext.clone()
    if scale_invariant:
        scale = 1 / near
        e[..., :3, 3] = e[..., :3, 3] * scale[:, None]
        near_s, far_s = near * scale, far * scale
    else:
        scale, near_s, far_s = torch.ones_like(near), near, far
    fov = sp.get_fov(intr)
    want = dict(tanfov=(0.5 * fov).tan(), view=torch.linalg.inv(e).transpose(1, 2), campos=e[:, :3, 3], scale=scale)
    want["full"] = want["view"] @ sp.get_projection_matrix(near_s, far_s, fov[:, 0], fov[:, 1], intr).transpose(1, 2)
    view, full, campos, tanfov, sc = cr.camera_setup_ref(ext, intr, near, far, scale_invariant)
    got = dict(view=view, full=full, campos=campos, tanfov=tanfov, scale=sc)
    for k, w in want.items():
        assert got[k].dtype == torch.float64 and got[k].shape == w.shape, k
        assert cr.rel_l2(w.numpy(), got[k].numpy()) < 2e-6, (k, cr.rel_l2(w.numpy(), got[k].numpy()))   # fp32 arithmetic of the branch
    # the cameras are what the GPU test needs: non-square, off-centre, every view its own
    assert (intr[:, 0, 2] - 0.5).abs().min() > 1e-4 and (intr[:, 0, 0] * 48 / 64 - intr[:, 1, 1] * 48 / 64).abs().min() > 0
    assert (tanfov[:, 0] / tanfov[:, 1] - 1).abs().min() > 0.01


def test_camera_reference_gradient_structure():
    """Row 0 of dL/dintrinsics carries the projection terms of ALL views, rows >= 1 only their own fov terms."""
    n = 3
    ext, intr, near, far = cr.cameras(n, seed=5)
    g = torch.Generator().manual_seed(0)
    k = intr.double().requires_grad_()
    view, full, campos, tanfov, _ = cr.camera_setup_ref(ext, k, near, far, True)
    (full * torch.randn(n, 4, 4, generator=g, dtype=torch.float64)).sum().backward()
    assert k.grad[0].abs().max() > 0 and float(k.grad[1:].abs().max()) == 0.0    # the projection reads intrinsics[0] alone
    k.grad = None
    view, full, campos, tanfov, _ = cr.camera_setup_ref(ext, k, near, far, True)
    (tanfov * torch.randn(n, 2, generator=g, dtype=torch.float64)).sum().backward()
    assert all(float(k.grad[i].abs().max()) > 0 for i in range(n))


# ---- the torch oracle differentiates tan(fov/2) --------------------------------------------------------------------------------
def test_torch_oracle_differentiates_tensor_tanfov():
    from ggrt_official_amd.synthetic import make_scene, upstream_gradient
    from oracle import torch_raster as tr
    sc = make_scene(300, 48, 32, sh_degree=1, seed=3)
    tx = torch.tensor(sc.tanfovx, dtype=torch.float64, requires_grad=True)
    ty = torch.tensor(sc.tanfovy, dtype=torch.float64, requires_grad=True)
    d = lambda t: t.double()
    color, radii, _ = tr.rasterize(d(sc.means3D), d(sc.opacities), d(sc.viewmatrix), d(sc.projmatrix), d(sc.campos), sc.bg, 48, 32,
                                   tx, ty, 1, shs=d(sc.shs), cov3D_precomp=d(sc.cov3D))
    ref, radii_f, _ = tr.rasterize(d(sc.means3D), d(sc.opacities), d(sc.viewmatrix), d(sc.projmatrix), d(sc.campos), sc.bg, 48, 32,
                                   sc.tanfovx, sc.tanfovy, 1, shs=d(sc.shs), cov3D_precomp=d(sc.cov3D))
    assert tx.dim() == 0 and torch.equal(radii, radii_f) and float((color.detach() - ref).abs().max()) < 1e-12
    (color * upstream_gradient(48, 32, seed=1).double()).sum().backward()
    for t in (tx, ty):
        assert t.grad is not None and bool(torch.isfinite(t.grad)) and float(t.grad.abs()) > 0.0


def test_reference_spread_on_dtanfov_is_below_a_quarter_of_the_bar():
    """The oracle's own fp32-against-fp64 difference on dL/dtanfov on the GPU test's scenes (the sums can cancel): one case
    per frame here, every case was measured when the seeds were chosen (tests/test_gpu_intrinsics_grad.py's docstring)."""
    from tests import tanfov_reference as R
    for frame in R.FRAMES:
        a = R.oracle64(frame, 0, "colour", False)
        b = R.oracle_grads(frame, 0, "colour", False, torch.float32)
        assert np.array_equal(a["radii"], b["radii"])
        s = cr.rel_l2(b["tanfov"], a["tanfov"])
        assert s < R.BAR / 4, (frame, s)


def test_launch_set_views_do_not_cancel():
    """The views of the GPU launch-set test are chosen by the cancellation of their dL/dtanfov sums (tests/tanfov_reference.py,
    `LS_VIEWS`): measured here again, per Gaussian on the oracle."""
    from tests import tanfov_reference as R
    seen = {}
    for (B, V), views in R.LS_VIEWS.items():
        bgs = R.ls_backgrounds(V)
        for v, (s, cam, up) in enumerate(views):
            seen[(B, V, v)] = R.ls_cancellation(s, cam, up, bgs[v])
    print({k: round(a, 2) for k, a in seen.items()})
    assert all(a < R.LS_MAX_CANCELLATION for a in seen.values()), seen

