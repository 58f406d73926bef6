"""The projection pass (ggr_projection / ggr_projection_backward, `return_projection`) — what needs no GPU: the symbols, the
layout of GgrProjectionPass against the compiled header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "reserved", "geom_buffer", "radii", "out_means2d", "out_depth", "out_conic", "out_opacity", "out_color",
          "out_valid", "dL_dmeans2d", "dL_ddepth", "dL_dconic", "dL_dopacity", "dL_dcolor", "scratch", "scratch_zeroed", "reserved2")
OUTPUTS, GRADS = FIELDS[4:10], FIELDS[10:15]


def test_symbols_exist():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ("ggr_projection", "ggr_projection_backward"):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob


def test_projection_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrHitPass", "GgrHitGradPass", "GgrPickPass", "GgrContributionPass", "GgrFeaturePass", "GgrDistortionPass",
              "GgrAbsgradPass", "GgrForwardExtra", "GgrBackwardExtra", "GgrBackwardExtra2", "GgrForwardOptions", "GgrSettings",
              "GgrViews", "GgrForwardIn", "GgrForwardOut", "GgrBackwardIn", "GgrBackwardOut")
    src = tmp_path / "pp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrProjectionPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrProjectionPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "pp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrProjectionPass) == size == 128
    assert int(lines[1]) == _lib.ABI_VERSION
    assert [f for f, _ in _lib.GgrProjectionPass._fields_] == list(FIELDS)
    for line in lines[2:2 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrProjectionPass, f).offset == int(off), f
    for line in lines[2 + len(FIELDS):2 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrHitPass) == 72   # (as it was)
    assert _lib.projection_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, geom_buffer=256, radii=256, scratch=256, scratch_zeroed=0, reserved2=0,
                **{f: 256 for f in OUTPUTS + GRADS})
    base.update(kw)
    return _lib.projection_pass(**base)


def _settings(**kw):
    return _lib.GgrSettings(**dict(dict(image_height=32, image_width=48, num_points=10), **kw))


BAD_FWD = [({f: None for f in OUTPUTS}, "all six outputs"), (dict(geom_buffer=None), "geom"), (dict(radii=None), "radii"),
           (dict(reserved=1), "reserved"), (dict(reserved2=7), "reserved")]
BAD_BWD = [({f: None for f in GRADS}, "all five gradients"), (dict(scratch=None), "scratch"), (dict(radii=None), "radii"),
           (dict(reserved=1), "reserved"), (dict(reserved2=7), "reserved")]


@pytest.mark.parametrize("fields,msg", BAD_FWD)
def test_invalid_forward_passes_are_refused_before_any_gpu_work(fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_projection(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrProjectionPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("fields,msg", BAD_BWD)
def test_invalid_backward_passes_are_refused_before_any_gpu_work(fields, msg):
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_projection_backward(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrProjectionPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry", ["ggr_projection", "ggr_projection_backward"])
def test_bad_struct_size_negative_sizes_and_views_are_refused(entry):
    lib = _lib.load()
    fn = getattr(lib, entry)
    st = _settings()
    for struct_size in (0, 8, -128, ctypes.sizeof(_lib.GgrProjectionPass) - 4):
        pp = _pass()
        pp.struct_size = struct_size
        assert fn(ctypes.byref(st), None, ctypes.byref(pp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    neg = _settings(num_points=-1)
    assert fn(ctypes.byref(neg), None, ctypes.byref(_pass()), None) == GGR_E_INVALID and "negative" in _lib.last_error()
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert fn(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID and "num_sets" in _lib.last_error()


def test_the_forward_with_no_gaussians_needs_no_gpu():
    """P = 0 is valid and enqueues nothing: the call returns GGR_OK in a process without a GPU"""
    lib = _lib.load()
    st = _settings(num_points=0)
    assert lib.ggr_projection(ctypes.byref(st), None, ctypes.byref(_pass(radii=None, **{f: None for f in OUTPUTS})), None) == 0
