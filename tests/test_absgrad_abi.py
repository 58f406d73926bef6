"""The absgrad pass (ggr_means2d_absgrad) — what needs no GPU: the symbol, the layout of GgrAbsgradPass against the compiled
header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "reserved", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "out_color", "out_depth",
          "dL_dout_color", "dL_dout_depth", "dL_dout_alpha", "out_absgrad", "out_grad")


def test_symbol_exists_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.ggr_means2d_absgrad is not None and "ggr_means2d_absgrad" in [s[0] for s in _lib.SYMBOLS]


def test_absgrad_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = {"GgrDistortionPass": 80, "GgrPickPass": 80, "GgrContributionPass": 64, "GgrForwardExtra": 16, "GgrBackwardExtra": 16}
    src = tmp_path / "ap.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(GgrAbsgradPass));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrAbsgradPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "ap"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrAbsgradPass) == size == 96
    assert [f for f, _ in _lib.GgrAbsgradPass._fields_] == list(FIELDS)
    for line in lines[1:1 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrAbsgradPass, f).offset == int(off), f
    for line in lines[1 + len(FIELDS):1 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n) == others[s], s
    assert _lib.absgrad_pass().struct_size == size


def _pass(**kw):
    base = dict(geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1, out_color=256, out_depth=256,
                dL_dout_color=256, dL_dout_depth=256, dL_dout_alpha=256, out_absgrad=256, out_grad=256)
    base.update(kw)
    return _lib.absgrad_pass(**base)


def _settings(**kw):
    return _lib.GgrSettings(**dict(dict(image_height=32, image_width=48, num_points=10), **kw))


BAD = [
    (dict(reserved=1), "reserved"),
    (dict(out_absgrad=None), "out_absgrad"),
    (dict(geom_buffer=None), "geom"),
    (dict(image_buffer=None), "geom"),
    (dict(binning_buffer=None), "binning_buffer"),
    (dict(out_color=None), "out_color"),
    (dict(dL_dout_color=None), "dL_dout_color"),
    (dict(out_depth=None), "out_depth"),          # … while dL_dout_depth is given
]


@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_means2d_absgrad(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrAbsgradPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("struct_size", [0, 8, -96, ctypes.sizeof(_lib.GgrAbsgradPass) - 4])
def test_bad_struct_size_is_refused(struct_size):
    lib = _lib.load()
    ap = _pass()
    ap.struct_size = struct_size
    st = _settings()
    assert lib.ggr_means2d_absgrad(ctypes.byref(st), None, ctypes.byref(ap), None) == GGR_E_INVALID
    assert "struct_size" in _lib.last_error()
    assert lib.ggr_means2d_absgrad(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    assert lib.ggr_means2d_absgrad(None, None, ctypes.byref(_pass()), None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert lib.ggr_means2d_absgrad(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()


def test_negative_sizes_are_refused_and_no_gaussians_is_nothing_to_do():
    lib = _lib.load()
    for kw in (dict(num_points=-1), dict(image_width=-1), dict(image_height=-1)):
        st = _settings(**kw)
        assert lib.ggr_means2d_absgrad(ctypes.byref(st), None, ctypes.byref(_pass()), None) == GGR_E_INVALID
        assert "negative" in _lib.last_error()
    st = _settings(num_points=0)   # P = 0: no row to clear, nothing to launch
    assert lib.ggr_means2d_absgrad(ctypes.byref(st), None, ctypes.byref(_pass()), None) == 0
