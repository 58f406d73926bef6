"""The ConvGRU gate math (ggr_gru_gate_forward / _blend_forward / _blend_backward / _gate_backward, `gru_gate`, `gru_blend`,
`fused_gru_half`, `FusedSepConvGRU`, `FusedConvGRU`) — what needs no GPU: the symbols, the layout of GgrGruPass against the compiled
header, the ABI version, the refusal of every invalid pass before any GPU work, and the refusals of the Python entry points that
are decided before a launch."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
POINTERS = ("a_zr_h", "a_zr_x", "h", "z", "r", "rh", "a_q_h", "a_q_x", "q", "out_h", "dL_dout_h", "dL_da_q", "dL_da_zr", "dL_dh_part", "dL_drh", "dL_dh")
# entry point: (required pointers, pointers that may be NULL, groups of outputs of which one must be given)
ENTRIES = {
    "ggr_gru_gate_forward": (("a_zr_h", "h", "z", "r", "rh"), ("a_zr_x",), ()),
    "ggr_gru_blend_forward": (("a_q_h", "z", "h", "q", "out_h"), ("a_q_x",), ()),
    "ggr_gru_blend_backward": (("dL_dout_h", "z", "q", "h"), (), ("dL_da_q", "dL_da_zr", "dL_dh_part")),
    "ggr_gru_gate_backward": (("dL_drh", "r", "h"), ("dL_dh_part",), ("dL_da_zr", "dL_dh")),
}


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES:
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    for kernel in (b"gru_gate_fwd_kernel", b"gru_blend_fwd_kernel", b"gru_blend_bwd_kernel", b"gru_gate_bwd_kernel"):
        assert kernel in blob          # (the device code is in the library)
    import ggrt_official_amd
    for name in ("gru_gate", "gru_blend", "fused_gru_half", "FusedSepConvGRU", "FusedConvGRU"):
        assert callable(getattr(ggrt_official_amd, name)) and name in ggrt_official_amd.__all__


def test_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrUpsampleDepthPass", "GgrWarpCostPass", "GgrPhotometricLossPass", "GgrImageLossPass", "GgrEpipolarAttnEncPass", "GgrEpipolarPass",
              "GgrDepthHeadPass", "GgrAdapterPass", "GgrSettings", "GgrViews")
    fields = [f for f, _ in _lib.GgrGruPass._fields_]
    assert tuple(fields[6:]) == POINTERS
    src = tmp_path / "gru.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrGruPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrGruPass, {f}));\n' for f in fields) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "gru"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrGruPass) == size == 152
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(fields)]:
        f, off = line.split()
        assert getattr(_lib.GgrGruPass, f).offset == int(off), f
    for line in lines[2 + len(fields):2 + len(fields) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrUpsampleDepthPass) == 112 and ctypes.sizeof(_lib.GgrWarpCostPass) == 168            # (as they were)
    assert _lib.gru_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, batch=2, channels=3, height=3, width=5, **{f: 256 + 16 * i for i, f in enumerate(POINTERS)})
    base.update(kw)
    return _lib.gru_pass(**base)


BAD = [(dict(batch=0), ".batch "), (dict(batch=-2), ".batch "), (dict(channels=0), ".channels "), (dict(channels=-1), ".channels "),
       (dict(height=0), ".height "), (dict(height=-7), ".height "), (dict(width=0), ".width "), (dict(width=-1), ".width "),
       (dict(reserved=1), "reserved"), (dict(reserved=-1), "reserved"), (dict(h=258), "misaligned"), (dict(h=257), "misaligned"),
       # N 2 M >= 2^31: exactly 2^31, far beyond it, and products that overflow 32 and 64 bits on the way
       (dict(batch=1, channels=1 << 10, height=1 << 10, width=1 << 10), "32-bit indexing"), (dict(batch=2, channels=128, height=2048, width=2048), "32-bit indexing"),
       (dict(batch=1 << 20, channels=1 << 20, height=1 << 20, width=1 << 20), "32-bit indexing"),
       (dict(batch=(1 << 31) - 1, channels=(1 << 31) - 1, height=(1 << 31) - 1, width=(1 << 31) - 1), "32-bit indexing")]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    rc = getattr(_lib.load(), entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrGruPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_null_required_pointers_bad_struct_sizes_and_missing_outputs_are_refused(entry):
    fn = getattr(_lib.load(), entry)
    required, optional, outputs = ENTRIES[entry]
    for f in required:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f"GgrGruPass.{f} is NULL" in _lib.last_error(), f
    for struct_size in (0, 8, -152, ctypes.sizeof(_lib.GgrGruPass) - 4):
        gp = _pass()
        gp.struct_size = struct_size
        assert fn(ctypes.byref(gp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrGruPass" in _lib.last_error()
    if outputs:
        assert fn(ctypes.byref(_pass(**{f: None for f in outputs})), None) == GGR_E_INVALID and "no output" in _lib.last_error()
    # a pointer the call does not use is not looked at: misaligned or NULL, the refusal that follows is the one of a used field
    unused = [f for f in POINTERS if f not in required + optional + outputs]
    gp = _pass(**{f: 3 for f in unused}, batch=0)
    assert fn(ctypes.byref(gp), None) == GGR_E_INVALID and ".batch " in _lib.last_error()
    gp = _pass(**{f: 3 for f in unused}, **{required[0]: 258})
    assert fn(ctypes.byref(gp), None) == GGR_E_INVALID and "misaligned" in _lib.last_error()


def test_the_blend_refuses_to_run_in_place():
    fn = _lib.load().ggr_gru_blend_forward
    assert fn(ctypes.byref(_pass(out_h=256 + 32, h=256 + 32)), None) == GGR_E_INVALID and "out_h is h itself" in _lib.last_error()


def test_python_entry_points_refuse_before_any_launch():
    from ggrt_official_amd import FusedConvGRU, FusedSepConvGRU, fused_gru_half, gru_blend, gru_gate
    route = "SepConvGRU.forward / ConvGRU.forward"
    h, x = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    w = (torch.zeros(6, 3, 1, 5), torch.zeros(6, 2, 1, 5), torch.zeros(6), torch.zeros(3, 3, 1, 5), torch.zeros(3, 2, 1, 5), torch.zeros(3))
    with pytest.raises(ValueError, match="h is on cpu.*GPU only.*" + route):
        fused_gru_half(h, x, *w, (0, 2))
    with pytest.raises(ValueError, match="x is torch.float16.*" + route):
        fused_gru_half(h, x.half(), *w, (0, 2))
    with pytest.raises(ValueError, match="w_q_h is torch.float64.*" + route):
        fused_gru_half(h, x, *w[:3], w[3].double(), *w[4:], (0, 2))
    with pytest.raises(ValueError, match="h is torch.float64.*" + route):
        FusedSepConvGRU(3, 2)(h.double(), x)
    with pytest.raises(ValueError, match="h is on cpu.*" + route):
        FusedConvGRU(3, 2)(h, x)
    with pytest.raises(ValueError, match="h is on cpu.*GPU only.*" + route):
        gru_gate(torch.zeros(2, 6, 4, 5), None, h)
    with pytest.raises(ValueError, match="a_zr_x is torch.float16.*" + route):
        gru_gate(torch.zeros(2, 6, 4, 5), torch.zeros(2, 6, 4, 5).half(), h)
    with pytest.raises(ValueError, match="z is torch.float64.*" + route):
        gru_blend(h, None, h.double(), h)
    with pytest.raises(ValueError, match="h is on cpu.*" + route):
        gru_blend(h, h, h, h)
    with pytest.raises(ValueError, match="not positive ints"):
        FusedSepConvGRU(0, 4)
