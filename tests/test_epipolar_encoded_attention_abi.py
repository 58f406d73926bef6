"""The encoded epipolar-attention pass (ggr_epipolar_attention_encoded_forward / _backward, `fused_epipolar_encoded_attention`) —
what needs no GPU: the symbols, the layout of GgrEpipolarAttnEncPass against the compiled header, and the refusal of every
invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = [f for f, _ in _lib.GgrEpipolarAttnEncPass._fields_]
FORWARD = ("qk", "qe", "features", "depth", "out_ctx_f", "out_ctx_e", "out_attn")
BACKWARD = ("qk", "qe", "features", "depth", "attn", "dL_dctx_f", "dL_dctx_e", "dL_dqk", "dL_dqe", "dL_dfeatures")
POINTERS = ("qk", "qe", "features", "depth", "out_ctx_f", "out_ctx_e", "out_attn", "attn", "dL_dctx_f", "dL_dctx_e", "dL_dqk", "dL_dqe",
            "dL_dfeatures", "dL_ddepth")
ENTRIES = ("ggr_epipolar_attention_encoded_forward", "ggr_epipolar_attention_encoded_backward")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES:
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    import ggrt_official_amd
    for name in ("fused_epipolar_encoded_attention", "epipolar_encoded_attention_core"):
        assert callable(getattr(ggrt_official_amd, name)) and name in ggrt_official_amd.__all__


def test_encoded_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrEpipolarAttnPass", "GgrEpipolarPass", "GgrDepthHeadPass", "GgrAdapterPass", "GgrProjectionPass", "GgrSettings", "GgrViews")
    assert FIELDS == ["struct_size", "reserved", "N", "S", "C", "H", "num_octaves", "reserved2"] + list(POINTERS)
    src = tmp_path / "ee.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrEpipolarAttnEncPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrEpipolarAttnEncPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "ee"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrEpipolarAttnEncPass) == size == 32 + 8 * len(POINTERS) == 144
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrEpipolarAttnEncPass, f).offset == int(off), f
    for line in lines[2 + len(FIELDS):2 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrEpipolarAttnPass) == 88 and ctypes.sizeof(_lib.GgrEpipolarPass) == 264      # (as they were)
    assert _lib.epipolar_attn_enc_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, N=3, S=8, C=16, H=4, num_octaves=10, reserved2=0, **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.epipolar_attn_enc_pass(**base)


BAD = [(dict(S=0), ".S "), (dict(S=65), ".S "), (dict(S=-1), ".S "), (dict(C=0), ".C "), (dict(C=257), ".C "), (dict(H=0), ".H "),
       (dict(H=9), ".H "), (dict(N=-1), ".N "), (dict(N=(1 << 25) + 1), ".N "), (dict(reserved=1), "reserved"), (dict(reserved2=1), "reserved"),
       (dict(num_octaves=0), ".num_octaves "), (dict(num_octaves=17), ".num_octaves "), (dict(num_octaves=-1), ".num_octaves "),
       (dict(qk=258), "misaligned"), (dict(qe=257), "misaligned"), (dict(features=257), "misaligned"), (dict(depth=259), "misaligned"),
       (dict(dL_dfeatures=259), "misaligned"), (dict(dL_ddepth=262), "misaligned"), (dict(out_ctx_e=262), "misaligned")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrEpipolarAttnEncPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_epipolar_attention_encoded_forward", FORWARD), ("ggr_epipolar_attention_encoded_backward", BACKWARD)])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    lib = _lib.load()
    fn = getattr(lib, entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -144, 88, ctypes.sizeof(_lib.GgrEpipolarAttnEncPass) - 4):
        ap = _pass()
        ap.struct_size = struct_size
        assert fn(ctypes.byref(ap), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrEpipolarAttnEncPass" in _lib.last_error()


def test_an_empty_call_needs_no_gpu():
    lib = _lib.load()
    nothing = {f: None for f in POINTERS}
    for entry in ENTRIES:
        fn = getattr(lib, entry)
        assert fn(ctypes.byref(_pass(N=0, **nothing)), None) == 0
        assert fn(ctypes.byref(_pass(N=0, S=64, C=256, H=8, num_octaves=16, **nothing)), None) == 0
        assert fn(ctypes.byref(_pass(N=0, S=65, **nothing)), None) == GGR_E_INVALID      # (scalars still checked)
        assert fn(ctypes.byref(_pass(N=0, num_octaves=0, **nothing)), None) == GGR_E_INVALID
        assert fn(ctypes.byref(_pass(N=0, reserved=2, **nothing)), None) == GGR_E_INVALID


def test_python_entry_points_refuse_cpu_tensors_bad_shapes_and_more_than_one_query_token():
    import torch
    from ggrt_official_amd import epipolar_encoded_attention_core, fused_epipolar_encoded_attention
    with pytest.raises(RuntimeError, match="GPU only"):
        epipolar_encoded_attention_core(torch.zeros(2, 1, 4), torch.zeros(2, 1, 6), torch.zeros(2, 3, 4), torch.zeros(2, 3))
    w = (torch.zeros(4, 6), torch.zeros(4), torch.zeros(4, 4), torch.zeros(8, 4), torch.zeros(4, 4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        fused_epipolar_encoded_attention(torch.zeros(2, 1, 4), torch.zeros(2, 3, 4), torch.zeros(2, 3), *w, heads=2)
    with pytest.raises(ValueError, match="ONE query token per ray"):
        fused_epipolar_encoded_attention(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), torch.zeros(2, 3), *w, heads=2)
