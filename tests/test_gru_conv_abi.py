"""The ConvGRU inference route (ggr_gru_conv_forward, ggr_gru_conv_workspace_bytes, `gru_conv`, `fused_gru_half_inference`, the
`hip_convs` flag) — what needs no GPU: the symbols, the layout of GgrGruConvPass against the compiled header, the ABI version, the
refusal of every invalid pass before any GPU work, and the refusals of the Python entry points that are decided before a launch."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
INTS = ("struct_size", "reserved", "batch", "channels", "in_channels", "height", "width", "kernel_h", "kernel_w", "epilogue", "out_channels")
POINTERS = ("a", "x", "w_h", "w_x", "bias", "h", "z", "rh", "out_h", "raw", "workspace")
GATE, BLEND, RAW = 0, 1, 2
# epilogue: (required pointers, pointers that may be NULL)
NEEDS = {GATE: (("a", "x", "w_h", "w_x", "h", "z", "rh"), ("bias", "workspace")), BLEND: (("a", "x", "w_h", "w_x", "h", "z", "out_h"), ("bias", "workspace")),
         RAW: (("a", "x", "w_h", "w_x", "raw"), ("bias", "workspace"))}


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ("ggr_gru_conv_forward", "ggr_gru_conv_workspace_bytes"):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    assert b"gru_conv_kernel" in blob          # (the device code is in the library)
    assert (_lib.GRU_CONV_GATE, _lib.GRU_CONV_BLEND, _lib.GRU_CONV_RAW) == (GATE, BLEND, RAW)
    import ggrt_official_amd
    for name in ("gru_conv", "fused_gru_half_inference"):
        assert callable(getattr(ggrt_official_amd, name)) and name in ggrt_official_amd.__all__


def test_the_new_source_is_built_and_hashed():
    from ggrt_official_amd import _build
    assert "gru_conv.hip" in _build.SOURCES and {"gru_conv.h", "gru_math.h"} <= set(_build.HEADERS)
    assert _build.embedded_hash() == _build.source_hash()


def test_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrGruPass", "GgrUpsampleDepthPass", "GgrWarpCostPass", "GgrPhotometricLossPass", "GgrImageLossPass", "GgrSettings", "GgrViews")
    fields = [f for f, _ in _lib.GgrGruConvPass._fields_]
    assert tuple(fields) == INTS + POINTERS + ("workspace_bytes",)
    src = tmp_path / "gru_conv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n%d %d %d\\n", sizeof(GgrGruConvPass), (int)GGR_ABI_VERSION, GGR_GRU_CONV_GATE, GGR_GRU_CONV_BLEND, GGR_GRU_CONV_RAW);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrGruConvPass, {f}));\n' for f in fields) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "gru_conv"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrGruConvPass) == size == 144
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    assert lines[2].split() == ["0", "1", "2"]
    for line in lines[3:3 + len(fields)]:
        f, off = line.split()
        assert getattr(_lib.GgrGruConvPass, f).offset == int(off), f
    for line in lines[3 + len(fields):3 + len(fields) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrGruPass) == 152 and ctypes.sizeof(_lib.GgrUpsampleDepthPass) == 112 and ctypes.sizeof(_lib.GgrWarpCostPass) == 168   # (as they were)
    assert _lib.gru_conv_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, batch=2, channels=3, in_channels=2, height=3, width=5, kernel_h=1, kernel_w=5, epilogue=GATE, out_channels=4, workspace_bytes=0,
                **{f: 256 + 16 * i for i, f in enumerate(POINTERS)})
    base.update(kw)
    return _lib.gru_conv_pass(**base)


BAD = [(dict(batch=0), ".batch "), (dict(batch=-2), ".batch "), (dict(channels=0), ".channels "), (dict(channels=-1), ".channels "),
       (dict(in_channels=0), ".in_channels "), (dict(in_channels=-3), ".in_channels "), (dict(height=0), ".height "), (dict(height=-7), ".height "),
       (dict(width=0), ".width "), (dict(width=-1), ".width "), (dict(reserved=1), "reserved"), (dict(reserved=-1), "reserved"),
       (dict(kernel_h=2), ".kernel_h 2"), (dict(kernel_h=0), ".kernel_h 0"), (dict(kernel_h=7), ".kernel_h 7"), (dict(kernel_h=-1), ".kernel_h -1"),
       (dict(kernel_w=4), ".kernel_w 4"), (dict(kernel_w=0), ".kernel_w 0"), (dict(kernel_w=7), ".kernel_w 7"), (dict(kernel_w=9), ".kernel_w 9"),
       (dict(a=258), "misaligned"), (dict(x=257), "misaligned"), (dict(w_h=259), "misaligned"), (dict(bias=2), "misaligned"), (dict(workspace=1), "misaligned"),
       (dict(workspace_bytes=-1), "workspace_bytes -1 is smaller"),
       # N 2 Ch H W >= 2^31: exactly 2^31, far beyond it, and products that overflow 32 and 64 bits on the way
       (dict(batch=1, channels=1 << 10, height=1 << 10, width=1 << 10), "32-bit indexing"), (dict(batch=2, channels=128, height=2048, width=2048), "32-bit indexing"),
       (dict(batch=1 << 20, channels=1 << 20, height=1 << 20, width=1 << 20), "32-bit indexing"),
       (dict(batch=(1 << 31) - 1, channels=(1 << 31) - 1, height=(1 << 31) - 1, width=(1 << 31) - 1), "32-bit indexing"),
       # ... and the other arrays of the call: x [N,Cx,H,W]
       (dict(batch=1, channels=1, in_channels=1 << 11, height=1 << 10, width=1 << 10), "32-bit indexing")]


@pytest.mark.parametrize("epilogue", [GATE, BLEND, RAW], ids=["gate", "blend", "raw"])
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(epilogue, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    rc = _lib.load().ggr_gru_conv_forward(ctypes.byref(_pass(epilogue=epilogue, **fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrGruConvPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("epilogue", [GATE, BLEND, RAW], ids=["gate", "blend", "raw"])
def test_null_required_pointers_bad_struct_sizes_and_unused_pointers(epilogue):
    fn = _lib.load().ggr_gru_conv_forward
    required, optional = NEEDS[epilogue]
    for f in required:
        assert fn(ctypes.byref(_pass(epilogue=epilogue, **{f: None})), None) == GGR_E_INVALID and f"GgrGruConvPass.{f} is NULL" in _lib.last_error(), f
    for struct_size in (0, 8, -144, ctypes.sizeof(_lib.GgrGruConvPass) - 4):
        cp = _pass(epilogue=epilogue)
        cp.struct_size = struct_size
        assert fn(ctypes.byref(cp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrGruConvPass" in _lib.last_error()
    # a pointer the epilogue does not use is not looked at: misaligned or NULL, the refusal that follows is the one of a used field
    unused = [f for f in POINTERS if f not in required + optional]
    cp = _pass(epilogue=epilogue, **{f: 3 for f in unused}, batch=0)
    assert fn(ctypes.byref(cp), None) == GGR_E_INVALID and ".batch " in _lib.last_error()
    cp = _pass(epilogue=epilogue, **{f: 3 for f in unused}, **{required[0]: 258})
    assert fn(ctypes.byref(cp), None) == GGR_E_INVALID and "misaligned" in _lib.last_error()
    cp = _pass(epilogue=epilogue, **{f: None for f in unused}, **{required[-1]: None})
    assert fn(ctypes.byref(cp), None) == GGR_E_INVALID and f".{required[-1]} is NULL" in _lib.last_error()


def test_unknown_epilogues_raw_without_columns_and_the_blend_in_place():
    fn = _lib.load().ggr_gru_conv_forward
    for e in (-1, 3, 17):
        assert fn(ctypes.byref(_pass(epilogue=e)), None) == GGR_E_INVALID and f".epilogue {e} " in _lib.last_error()
    for c in (0, -4):
        assert fn(ctypes.byref(_pass(epilogue=RAW, out_channels=c)), None) == GGR_E_INVALID and f".out_channels {c} " in _lib.last_error()
    for e in (GATE, BLEND):          # (implied by Ch: not looked at)
        assert fn(ctypes.byref(_pass(epilogue=e, out_channels=-4, batch=0)), None) == GGR_E_INVALID and ".batch " in _lib.last_error()
    assert fn(ctypes.byref(_pass(epilogue=BLEND, out_h=256 + 32, h=256 + 32)), None) == GGR_E_INVALID and "out_h is h itself" in _lib.last_error()
    # raw [N,Cout,H,W] beyond 2^31 - 1 elements
    assert fn(ctypes.byref(_pass(epilogue=RAW, out_channels=1 << 30)), None) == GGR_E_INVALID and "32-bit indexing" in _lib.last_error()


def test_workspace_bytes_is_zero_for_every_pass():
    fn = _lib.load().ggr_gru_conv_workspace_bytes
    assert fn(None) == 0
    for e in (GATE, BLEND, RAW):
        for dims in (dict(), dict(batch=1, channels=128, in_channels=160, height=48, width=63), dict(batch=5, channels=128, in_channels=160, height=48, width=63)):
            assert fn(ctypes.byref(_pass(epilogue=e, **dims))) == 0


def test_python_entry_points_refuse_before_any_launch():
    from ggrt_official_amd import FusedConvGRU, FusedSepConvGRU, fused_gru_half_inference, gru_conv
    torch_route, train_route = "SepConvGRU.forward / ConvGRU.forward", "use fused_gru_half "
    h, x = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    w = (torch.zeros(6, 3, 1, 5), torch.zeros(6, 2, 1, 5), torch.zeros(6), torch.zeros(3, 3, 1, 5), torch.zeros(3, 2, 1, 5), torch.zeros(3))
    with pytest.raises(ValueError, match="fused_gru_half_inference: h is on cpu.*GPU only.*" + torch_route):
        fused_gru_half_inference(h, x, *w, (0, 2))
    with pytest.raises(ValueError, match="fused_gru_half_inference: x is torch.float16.*" + torch_route):
        fused_gru_half_inference(h, x.half(), *w, (0, 2))
    with pytest.raises(ValueError, match="w_q_h is torch.float64.*" + torch_route):
        fused_gru_half_inference(h, x, *w[:3], w[3].double(), *w[4:], (0, 2))
    with pytest.raises(ValueError, match="gru_conv: a is on cpu.*GPU only.*" + train_route):
        gru_conv(h, x, w[0], w[1], w[2], (0, 2))
    with pytest.raises(ValueError, match="gru_conv: w_x is torch.float64.*" + train_route):
        gru_conv(h, x, w[0], w[1].double(), w[2], (0, 2))
    for cls in (FusedSepConvGRU, FusedConvGRU):
        assert cls(3, 2).hip_convs is False and cls(3, 2, hip_convs=True).hip_convs is True
        with pytest.raises(TypeError):
            cls(3, 2, True)
        with torch.no_grad(), pytest.raises(ValueError, match="fused_gru_half_inference: h is on cpu.*" + torch_route):
            cls(3, 2, hip_convs=True)(h, x)
        with pytest.raises(ValueError, match="fused_gru_half: h is on cpu.*" + torch_route):
            cls(3, 2, hip_convs=True)(h, x)          # (parameters require grad: the training route)
        assert sorted(cls(3, 2, hip_convs=True).state_dict()) == sorted(cls(3, 2).state_dict())
