"""The pick pass (ggr_pixel_picks, `return_picks`) — what needs no GPU: the symbol, the layout of GgrPickPass against the
compiled header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "reserved", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "out_median_index",
          "out_median_depth", "out_max_index", "out_max_weight", "out_count")
OUTPUTS = FIELDS[6:]


def test_symbol_exists_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.ggr_pixel_picks is not None and "ggr_pixel_picks" in [s[0] for s in _lib.SYMBOLS]


def test_pick_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrContributionPass", "GgrFeaturePass", "GgrForwardExtra", "GgrBackwardExtra", "GgrForwardOptions", "GgrSettings",
              "GgrViews", "GgrForwardIn", "GgrForwardOut", "GgrBackwardIn", "GgrBackwardOut")
    src = tmp_path / "pp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(GgrPickPass));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrPickPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "pp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrPickPass) == size == 80
    assert [f for f, _ in _lib.GgrPickPass._fields_] == list(FIELDS)
    for line in lines[1:1 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrPickPass, f).offset == int(off), f
    for line in lines[1 + len(FIELDS):1 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrContributionPass) == 64   # (as it was)
    assert _lib.pick_pass().struct_size == size


def _pass(**kw):
    base = dict(geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1, **{f: 256 for f in OUTPUTS})
    base.update(kw)
    return _lib.pick_pass(**base)


def _settings():
    return _lib.GgrSettings(image_height=32, image_width=48, num_points=10)


BAD = [
    (dict(reserved=1), "reserved"),
    ({f: None for f in OUTPUTS}, "every output is NULL"),
    (dict(geom_buffer=None), "geom"),
    (dict(image_buffer=None), "geom"),
    (dict(binning_buffer=None), "binning_buffer"),
]


@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_pixel_picks(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrPickPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("struct_size", [0, 8, -80, ctypes.sizeof(_lib.GgrPickPass) - 4])
def test_bad_struct_size_is_refused(struct_size):
    lib = _lib.load()
    pp = _pass()
    pp.struct_size = struct_size
    st = _settings()
    assert lib.ggr_pixel_picks(ctypes.byref(st), None, ctypes.byref(pp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert lib.ggr_pixel_picks(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert lib.ggr_pixel_picks(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()
