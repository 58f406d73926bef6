"""The hit pass (ggr_pixel_hits, `return_hits`) — what needs no GPU: the symbol, the layout of GgrHitPass and GGR_MAX_HITS
against the compiled header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "num_hits", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "out_index", "out_weight",
          "out_rest", "out_count")
OUTPUTS = FIELDS[6:]


def test_symbol_exists_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.ggr_pixel_hits is not None and "ggr_pixel_hits" in [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"ggr_pixel_hits" in f.read()


def test_hit_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrPickPass", "GgrContributionPass", "GgrFeaturePass", "GgrDistortionPass", "GgrAbsgradPass", "GgrForwardExtra",
              "GgrBackwardExtra", "GgrForwardOptions", "GgrSettings", "GgrViews", "GgrForwardIn", "GgrForwardOut", "GgrBackwardIn",
              "GgrBackwardOut")
    src = tmp_path / "hp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n%d\\n", sizeof(GgrHitPass), (int)GGR_MAX_HITS, (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrHitPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "hp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrHitPass) == size == 72
    assert int(lines[1]) == _lib.MAX_HITS == 32 and int(lines[2]) == _lib.ABI_VERSION
    assert [f for f, _ in _lib.GgrHitPass._fields_] == list(FIELDS)
    for line in lines[3:3 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrHitPass, f).offset == int(off), f
    for line in lines[3 + len(FIELDS):3 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrPickPass) == 80 and ctypes.sizeof(_lib.GgrContributionPass) == 64   # (as they were)
    assert _lib.hit_pass().struct_size == size


def _pass(**kw):
    base = dict(num_hits=4, geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1, **{f: 256 for f in OUTPUTS})
    base.update(kw)
    return _lib.hit_pass(**base)


def _settings():
    return _lib.GgrSettings(image_height=32, image_width=48, num_points=10)


BAD = [
    (dict(num_hits=0), "num_hits"),
    (dict(num_hits=-1), "num_hits"),
    (dict(num_hits=_lib.MAX_HITS + 1), "num_hits"),
    (dict(out_index=None), "pair"),
    (dict(out_weight=None), "pair"),
    (dict(out_index=None, out_rest=None, out_count=None), "pair"),
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
    rc = lib.ggr_pixel_hits(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrHitPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("struct_size", [0, 8, -72, ctypes.sizeof(_lib.GgrHitPass) - 4])
def test_bad_struct_size_is_refused(struct_size):
    lib = _lib.load()
    hp = _pass()
    hp.struct_size = struct_size
    st = _settings()
    assert lib.ggr_pixel_hits(ctypes.byref(st), None, ctypes.byref(hp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert lib.ggr_pixel_hits(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert lib.ggr_pixel_hits(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()
