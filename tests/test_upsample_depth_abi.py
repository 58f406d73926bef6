"""The convex depth upsampling pass (ggr_upsample_depth_forward / _backward, `fused_upsample_depth`) — what needs no GPU: the
symbols, the layout of GgrUpsampleDepthPass against the compiled header, the ABI version, the refusal of every invalid pass before
any GPU work, the size query, and the refusals of the Python entry point, each naming the argument and the torch route."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
ENTRIES = ("ggr_upsample_depth_forward", "ggr_upsample_depth_backward")
FORWARD = ("depth", "mask", "out", "workspace")
BACKWARD = ("depth", "mask", "dL_dout", "workspace")
POINTERS = ("depth", "mask", "out", "workspace", "dL_dout", "dL_dmask", "dL_ddepth")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES + ("ggr_upsample_depth_workspace_bytes",):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    for kernel in (b"upsample_convex_kernel", b"upsample_resize_kernel", b"upsample_cells_bwd_kernel", b"upsample_depth_bwd_kernel"):
        assert kernel in blob          # (the device code is in the library)
    import ggrt_official_amd
    assert callable(ggrt_official_amd.fused_upsample_depth) and "fused_upsample_depth" in ggrt_official_amd.__all__


def test_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrWarpCostPass", "GgrPhotometricLossPass", "GgrImageLossPass", "GgrEpipolarAttnEncPass", "GgrEpipolarPass", "GgrDepthHeadPass", "GgrAdapterPass",
              "GgrSettings", "GgrViews")
    fields = [f for f, _ in _lib.GgrUpsampleDepthPass._fields_]
    src = tmp_path / "ud.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrUpsampleDepthPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrUpsampleDepthPass, {f}));\n' for f in fields) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "ud"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrUpsampleDepthPass) == size == 112
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(fields)]:
        f, off = line.split()
        assert getattr(_lib.GgrUpsampleDepthPass, f).offset == int(off), f
    for line in lines[2 + len(fields):2 + len(fields) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrWarpCostPass) == 168 and ctypes.sizeof(_lib.GgrPhotometricLossPass) == 208            # (as they were)
    assert _lib.upsample_depth_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, batch=2, height=6, width=10, ratio=8, out_height=45, out_width=80, fold_disp=0, reserved2=0, min_depth=0.0, max_depth=0.0,
                workspace_bytes=1 << 24, **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.upsample_depth_pass(**base)


BIG = 1 << 16
BAD = [(dict(ratio=0), ".ratio "), (dict(ratio=-1), ".ratio "), (dict(ratio=9), ".ratio "), (dict(batch=0), ".batch "), (dict(batch=-3), ".batch "),
       (dict(height=0), ".height "), (dict(width=0), ".width "), (dict(out_height=0), ".out_height "), (dict(out_width=0), ".out_width "),
       (dict(out_width=-5), ".out_width "), (dict(fold_disp=2), ".fold_disp "), (dict(fold_disp=-1), ".fold_disp "),
       (dict(fold_disp=1), ".min_depth "), (dict(fold_disp=1, min_depth=0.0, max_depth=100.0), ".min_depth "),
       (dict(fold_disp=1, min_depth=-1.0, max_depth=100.0), ".min_depth "), (dict(fold_disp=1, min_depth=2.0, max_depth=1.0), ".min_depth "),
       (dict(fold_disp=1, min_depth=1.0, max_depth=1.0), ".min_depth "), (dict(fold_disp=1, min_depth=1.0, max_depth=float("inf")), ".max_depth "),
       (dict(fold_disp=1, min_depth=float("nan"), max_depth=2.0), ".min_depth "), (dict(reserved=1), "reserved"), (dict(reserved2=1), "reserved"),
       (dict(depth=258), "misaligned"), (dict(mask=257), "misaligned"), (dict(workspace=259), "misaligned"),
       (dict(workspace_bytes=2 * 6 * 10 * 64 * 4 - 1), "workspace_bytes"),
       # sizes beyond 32-bit indexing: the mask's element count, the output's, a side of `up`, a side of the output
       (dict(batch=64, height=1024, width=1024, ratio=2), "32-bit indexing"), (dict(batch=1, height=2048, width=2048, ratio=8), "32-bit indexing"),
       (dict(batch=40000, height=4, width=4, ratio=1, out_height=BIG // 2, out_width=BIG // 2), "32-bit indexing"),
       (dict(batch=1, height=BIG // 8 + 1, width=1, ratio=8), "32-bit indexing"), (dict(out_height=BIG + 1, out_width=1), "32-bit indexing")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrUpsampleDepthPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_upsample_depth_forward", FORWARD), ("ggr_upsample_depth_backward", BACKWARD)])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    fn = getattr(_lib.load(), entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -128, ctypes.sizeof(_lib.GgrUpsampleDepthPass) - 4):
        up = _pass()
        up.struct_size = struct_size
        assert fn(ctypes.byref(up), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrUpsampleDepthPass" in _lib.last_error()


def test_a_backward_without_any_output_is_refused():
    fn = _lib.load().ggr_upsample_depth_backward
    assert fn(ctypes.byref(_pass(dL_dmask=None, dL_ddepth=None)), None) == GGR_E_INVALID and "no output" in _lib.last_error()


def test_the_size_query():
    q = _lib.load().ggr_upsample_depth_workspace_bytes
    assert q(4, 48, 63, 8) == 4 * 48 * 63 * 64 * 4          # `up`: 384 x 504 per map
    assert q(1, 1, 1, 2) == 9 * 4 and q(2, 4, 7, 1) == 2 * 4 * 7 * 9 * 4 and q(1, 3, 70, 3) == 3 * 70 * 9 * 4          # the tap sums where r r < 9
    assert q(1, 5, 5, 8) > 0 and q(1, 5, 5, 9) == -1 and q(1, 5, 5, 0) == -1
    assert q(0, 5, 5, 8) == -1 and q(1, 0, 5, 8) == -1 and q(1, 5, -1, 8) == -1
    assert q(1, 2048, 2048, 8) == -1 and q(1, 1920, 1920, 8) > 0          # 9 x 64 x 2048^2 > 2^31 - 1 >= 9 x 64 x 1920^2
    assert q(1, BIG // 8, 1, 8) > 0 and q(1, BIG // 8 + 1, 1, 8) == -1


def test_python_entry_point_refuses_before_any_launch():
    from ggrt_official_amd import fused_upsample_depth
    route = "DepthPoseNet.upsample_depth"
    d, m = torch.zeros(2, 1, 3, 4), torch.zeros(2, 576, 3, 4)
    with pytest.raises(ValueError, match="depth is on cpu.*GPU only.*" + route):
        fused_upsample_depth(d, m)
    with pytest.raises(ValueError, match="mask is torch.float16.*" + route):
        fused_upsample_depth(d, m.half())
    with pytest.raises(ValueError, match="depth is torch.float64.*" + route):
        fused_upsample_depth(d.double(), m)
    with pytest.raises(ValueError, match="ratio 9.*" + route):
        fused_upsample_depth(d, m, ratio=9)
    with pytest.raises(ValueError, match="ratio 0.*" + route):
        fused_upsample_depth(d, m, ratio=0)
    with pytest.raises(ValueError, match="disp_range.*0 < min < max.*" + route):
        fused_upsample_depth(d, m, disp_range=(100.0, 0.1))
    with pytest.raises(ValueError, match="both be tensors or both be lists.*" + route):
        fused_upsample_depth([d], m)
    with pytest.raises(ValueError, match="empty or differ in length.*" + route):
        fused_upsample_depth([d, d], [m])
    with pytest.raises(ValueError, match="empty or differ in length.*" + route):
        fused_upsample_depth([], [])
