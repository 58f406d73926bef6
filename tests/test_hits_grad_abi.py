"""The hit pass's backward (ggr_pixel_hits_backward, `hits_grad`) — what needs no GPU: the symbol, the layout of GgrHitGradPass
against the compiled header, GgrHitPass and every other struct unchanged, and the refusal of every invalid pass before any GPU
work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "num_hits", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "weight", "rest", "count",
          "dL_dweight", "dL_drest", "scratch", "scratch_zeroed", "reserved")
POINTERS = ("geom_buffer", "image_buffer", "binning_buffer", "weight", "rest", "count", "dL_dweight", "dL_drest", "scratch")


def test_symbol_exists_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.ggr_pixel_hits_backward is not None and "ggr_pixel_hits_backward" in [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"ggr_pixel_hits_backward" in f.read()
    assert "blend_hits_grad.hip" in _build.SOURCES and "blend_hits_grad.h" in _build.HEADERS
    assert _build.EXTRA_FLAGS["blend_hits_grad.hip"] == _build.EXTRA_FLAGS["blend_hits.hip"]


def test_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrHitPass", "GgrPickPass", "GgrContributionPass", "GgrFeaturePass", "GgrDistortionPass", "GgrAbsgradPass",
              "GgrForwardExtra", "GgrBackwardExtra", "GgrForwardOptions", "GgrSettings", "GgrViews", "GgrForwardIn", "GgrForwardOut",
              "GgrBackwardIn", "GgrBackwardOut")
    src = tmp_path / "hg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n%d\\n", sizeof(GgrHitGradPass), (int)GGR_MAX_HITS, (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrHitGradPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "hg"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrHitGradPass) == size == 96
    assert int(lines[1]) == _lib.MAX_HITS == 32 and int(lines[2]) == _lib.ABI_VERSION
    assert [f for f, _ in _lib.GgrHitGradPass._fields_] == list(FIELDS)
    for line in lines[3:3 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrHitGradPass, f).offset == int(off), f
    for line in lines[3 + len(FIELDS):3 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrHitPass) == 72   # (as it was)
    assert [f for f, _ in _lib.GgrHitPass._fields_] == ["struct_size", "num_hits", "geom_buffer", "image_buffer", "binning_buffer",
                                                         "num_rendered", "out_index", "out_weight", "out_rest", "out_count"]
    assert _lib.hit_grad_pass().struct_size == size


def _pass(**kw):
    base = dict(num_hits=4, num_rendered=1, scratch_zeroed=0, reserved=0, **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.hit_grad_pass(**base)


def _settings(**kw):
    return _lib.GgrSettings(**dict(dict(image_height=32, image_width=48, num_points=10), **kw))


BAD = [
    (dict(num_hits=0), "num_hits"),
    (dict(num_hits=-1), "num_hits"),
    (dict(num_hits=_lib.MAX_HITS + 1), "num_hits"),
    (dict(reserved=1), "reserved"),
    (dict(dL_dweight=None, dL_drest=None), "both NULL"),
    (dict(geom_buffer=None), "geom"),
    (dict(image_buffer=None), "geom"),
    (dict(binning_buffer=None), "binning_buffer"),
    (dict(weight=None), "weight is NULL"),
    (dict(weight=None, dL_dweight=None), "weight is NULL"),   # (required whichever gradient comes)
    (dict(count=None), "count is NULL"),
    (dict(scratch=None), "scratch is NULL"),
]


@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_pixel_hits_backward(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrHitGradPass" in _lib.last_error(), (rc, _lib.last_error())


def test_negative_sizes_null_arguments_and_bad_view_sets_are_refused():
    lib = _lib.load()
    for bad in (dict(num_points=-1), dict(image_width=-1), dict(image_height=-1)):
        st = _settings(**bad)
        assert lib.ggr_pixel_hits_backward(ctypes.byref(st), None, ctypes.byref(_pass()), None) == GGR_E_INVALID
        assert "negative size" in _lib.last_error()
    st = _settings()
    assert lib.ggr_pixel_hits_backward(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    assert lib.ggr_pixel_hits_backward(None, None, ctypes.byref(_pass()), None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert lib.ggr_pixel_hits_backward(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()
    vw = _lib.GgrViews(num_views=0)
    assert lib.ggr_pixel_hits_backward(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID


@pytest.mark.parametrize("struct_size", [0, 8, -96, 72, ctypes.sizeof(_lib.GgrHitGradPass) - 4])
def test_bad_struct_size_is_refused(struct_size):
    lib = _lib.load()
    hp = _pass()
    hp.struct_size = struct_size
    st = _settings()
    assert lib.ggr_pixel_hits_backward(ctypes.byref(st), None, ctypes.byref(hp), None) == GGR_E_INVALID
    assert "struct_size" in _lib.last_error()


def test_a_missing_gradient_or_rest_is_accepted_by_the_validation():
    """One of the two gradients NULL, and `rest` NULL (it is not read), pass the checks: the call gets as far as its first HIP call, which
    fails in a process without a GPU — with another code and text than a refusal."""
    lib = _lib.load()
    st = _settings()
    for fields in (dict(dL_drest=None), dict(rest=None), dict(dL_drest=None, rest=None), dict(dL_dweight=None)):
        rc = lib.ggr_pixel_hits_backward(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
        assert rc != GGR_E_INVALID or "GgrHitGradPass" not in _lib.last_error(), (fields, rc, _lib.last_error())
