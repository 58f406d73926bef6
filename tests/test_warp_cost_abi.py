"""The cost-map pass (ggr_warp_cost_forward / _backward, `fused_warp_cost`) — what needs no GPU: the symbols, the layout of
GgrWarpCostPass against the compiled header, the ABI version, the refusal of every invalid pass before any GPU work, the size query,
and the refusals of the Python entry point, each naming the argument and the torch route."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
ENTRIES = ("ggr_warp_cost_forward", "ggr_warp_cost_backward")
INPUTS = ("fmap", "fmaps_ref", "inv_depth", "K", "ref_Ks", "poses")
FORWARD = INPUTS + ("out_cost",)
BACKWARD = INPUTS + ("dL_dcost", "workspace")
POINTERS = INPUTS + ("out_cost", "out_cells", "workspace", "dL_dcost", "dL_dfmap", "dL_dfmaps_ref", "dL_dinv_depth", "dL_dposes")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES + ("ggr_warp_cost_workspace_bytes",):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    assert b"warp_cost_fwd_kernel" in blob and b"warp_cost_bwd_kernel" in blob          # (the device code is in the library)
    import ggrt_official_amd
    assert callable(ggrt_official_amd.fused_warp_cost) and "fused_warp_cost" in ggrt_official_amd.__all__


def test_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrPhotometricLossPass", "GgrImageLossPass", "GgrEpipolarAttnEncPass", "GgrEpipolarPass", "GgrDepthHeadPass", "GgrAdapterPass", "GgrSettings", "GgrViews")
    fields = [f for f, _ in _lib.GgrWarpCostPass._fields_]
    src = tmp_path / "wc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrWarpCostPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrWarpCostPass, {f}));\n' for f in fields) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "wc"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrWarpCostPass) == size == 168
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(fields)]:
        f, off = line.split()
        assert getattr(_lib.GgrWarpCostPass, f).offset == int(off), f
    for line in lines[2 + len(fields):2 + len(fields) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrPhotometricLossPass) == 208            # (as it was)
    assert _lib.warp_cost_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, num_views=2, channels=5, height=20, width=40, reduce_mean=1, fold_disp=0, scale_factor=0.125, min_depth=0.0, max_depth=0.0,
                reserved2=0, workspace_bytes=1 << 24, **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.warp_cost_pass(**base)


BAD = [(dict(num_views=0), ".num_views "), (dict(num_views=-1), ".num_views "), (dict(num_views=17), ".num_views "), (dict(channels=0), ".channels "),
       (dict(channels=65537), ".channels "), (dict(height=1), ".height "), (dict(width=1), ".width "), (dict(height=16385), ".height "),
       (dict(width=16385), ".width "), (dict(reduce_mean=2), ".reduce_mean "), (dict(fold_disp=-1), ".fold_disp "),
       (dict(scale_factor=0.0), ".scale_factor "), (dict(scale_factor=-0.125), ".scale_factor "), (dict(scale_factor=float("nan")), ".scale_factor "),
       (dict(scale_factor=float("inf")), ".scale_factor "), (dict(fold_disp=1), ".min_depth "), (dict(fold_disp=1, min_depth=2.0, max_depth=1.0), ".min_depth "),
       (dict(fold_disp=1, min_depth=1.0, max_depth=1.0), ".min_depth "), (dict(fold_disp=1, min_depth=1.0, max_depth=float("inf")), ".max_depth "),
       (dict(fold_disp=1, min_depth=float("nan"), max_depth=2.0), ".min_depth "), (dict(reserved=1), "reserved"), (dict(reserved2=1), "reserved"),
       (dict(fmap=258), "misaligned"), (dict(poses=257), "misaligned"), (dict(out_cells=259), "misaligned")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrWarpCostPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_warp_cost_forward", FORWARD), ("ggr_warp_cost_backward", BACKWARD)])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    fn = getattr(_lib.load(), entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -128, ctypes.sizeof(_lib.GgrWarpCostPass) - 4):
        wp = _pass()
        wp.struct_size = struct_size
        assert fn(ctypes.byref(wp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrWarpCostPass" in _lib.last_error()


def test_backward_refusals_of_its_own():
    fn = _lib.load().ggr_warp_cost_backward
    none = dict(dL_dfmap=None, dL_dfmaps_ref=None, dL_dinv_depth=None, dL_dposes=None)
    assert fn(ctypes.byref(_pass(**none)), None) == GGR_E_INVALID and "no output" in _lib.last_error()
    assert fn(ctypes.byref(_pass(workspace_bytes=64)), None) == GGR_E_INVALID and "workspace_bytes" in _lib.last_error()
    assert fn(ctypes.byref(_pass(workspace=260)), None) == GGR_E_INVALID and "workspace is misaligned" in _lib.last_error()


def test_the_size_query():
    lib = _lib.load()
    assert lib.ggr_warp_cost_workspace_bytes(5, 48, 63) == 48 * 5 * 12 * 8          # 3024 pixels: 47.25 tiles of 64
    assert lib.ggr_warp_cost_workspace_bytes(1, 2, 2) == 1 * 1 * 12 * 8 and lib.ggr_warp_cost_workspace_bytes(2, 5, 13) == 2 * 2 * 12 * 8
    assert lib.ggr_warp_cost_workspace_bytes(16, 8, 8) > 0 and lib.ggr_warp_cost_workspace_bytes(17, 8, 8) == -1
    assert lib.ggr_warp_cost_workspace_bytes(0, 8, 8) == -1 and lib.ggr_warp_cost_workspace_bytes(1, 1, 8) == -1 and lib.ggr_warp_cost_workspace_bytes(1, 8, 16385) == -1


def test_python_entry_point_refuses_before_any_launch():
    from ggrt_official_amd import fused_warp_cost
    V, C, h, w = 2, 3, 4, 5
    mk = lambda: [torch.zeros(1, C, h, w), torch.zeros(V, C, h, w), torch.ones(1, 1, h, w), torch.eye(3)[None], torch.eye(3).repeat(V, 1, 1), torch.zeros(V, 6)]
    route = "get_cost_each"
    with pytest.raises(ValueError, match="fmap is on cpu.*GPU only.*" + route):
        fused_warp_cost(*mk())
    a = mk()
    a[5] = a[5].half()
    with pytest.raises(ValueError, match="poses is torch.float16.*" + route):
        fused_warp_cost(*a)
    with pytest.raises(ValueError, match="reduce 'max'.*" + route):
        fused_warp_cost(*mk(), reduce="max")
    with pytest.raises(ValueError, match="scale_factor.*" + route):
        fused_warp_cost(*mk(), scale_factor=0)
    with pytest.raises(ValueError, match="disp_range.*0 < min < max.*" + route):
        fused_warp_cost(*mk(), disp_range=(100.0, 0.1))
    a = mk()
    a[1] = []
    with pytest.raises(ValueError, match="V = 0.*" + route):
        fused_warp_cost(*a)
    a = mk()
    a[1] = [torch.zeros(1, C, h, w), torch.zeros(1, C, h, w + 1)]
    with pytest.raises(ValueError, match="fmaps_ref.*spatial sizes.*" + route):
        fused_warp_cost(*a)
    a = mk()
    a[5] = [torch.zeros(2, 6)]
    with pytest.raises(ValueError, match="poses.*batch other than 1.*" + route):
        fused_warp_cost(*a)
