"""The epipolar-sampler pass (ggr_epipolar_forward / ggr_epipolar_backward, `fused_epipolar_sampler`) — what needs no GPU: the
symbols, the layout of GgrEpipolarPass against the compiled header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = [f for f, _ in _lib.GgrEpipolarPass._fields_]
CAMERAS = ("c2w", "w2c", "K", "Kinv", "near", "far")
OUTPUTS = ("features", "valid", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions", "depth", "segment")
BACKWARD = ("dL_dfeatures", "dL_dimages")
POINTERS = CAMERAS + ("images",) + OUTPUTS + BACKWARD + ("scratch",)
ENTRIES = ("ggr_epipolar_forward", "ggr_epipolar_backward")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES + ("ggr_epipolar_scratch_bytes",):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    import ggrt_official_amd
    assert callable(ggrt_official_amd.fused_epipolar_sampler) and "fused_epipolar_sampler" in ggrt_official_amd.__all__


def test_epipolar_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrDepthHeadPass", "GgrAdapterPass", "GgrProjectionPass", "GgrHitPass", "GgrSettings", "GgrViews")
    assert FIELDS[:2] == ["struct_size", "reserved"] and set(POINTERS) < set(FIELDS)
    src = tmp_path / "ep.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrEpipolarPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrEpipolarPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "ep"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrEpipolarPass) == size == 264
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrEpipolarPass, f).offset == int(off), f
    for line in lines[2 + len(FIELDS):2 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrDepthHeadPass) == 184 and ctypes.sizeof(_lib.GgrAdapterPass) == 248      # (as they were)
    assert _lib.epipolar_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, batch=1, num_views=2, channels=16, height=6, width=8, num_samples=8, use_window=0, window_y0=0,
                window_y1=0, window_x0=0, window_x1=0, debug=0, image_strides=(2 * 16 * 48, 16 * 48, 48, 8, 1),
                scratch_bytes=1 * 2 * 16 * 48 * 4, **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.epipolar_pass(**base)


BAD = [(dict(num_samples=0), "num_samples"), (dict(num_samples=65), "num_samples"), (dict(channels=0), "channels"),
       (dict(channels=513), "channels"), (dict(num_views=1), "num_views"), (dict(num_views=9), "num_views"),
       (dict(batch=-1), "batch"), (dict(height=0), "height"), (dict(width=-4), "width"), (dict(reserved=1), "reserved"),
       (dict(use_window=1), "window"), (dict(use_window=1, window_y0=2, window_y1=2, window_x1=3), "window"),
       (dict(use_window=1, window_y1=7, window_x1=3), "window"), (dict(use_window=1, window_y1=3, window_x0=-1, window_x1=3), "window"),
       (dict(use_window=1, window_y1=3, window_x1=9), "window"),
       (dict(batch=8192, num_views=8, scratch_bytes=1 << 62), "too large"),
       (dict(batch=4096, height=1 << 12, width=1 << 12, scratch_bytes=1 << 62), "too large"),
       (dict(batch=2048, num_views=8, height=128, width=128, num_samples=64, scratch_bytes=1 << 62), "too large"),
       (dict(scratch_bytes=1 * 2 * 16 * 48 * 4 - 4), "scratch_bytes"), (dict(scratch=None), "scratch"),
       (dict(K=258), "misaligned"), (dict(segment=257), "misaligned"), (dict(dL_dimages=259), "misaligned")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrEpipolarPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_epipolar_forward", CAMERAS + ("images",)),
                                          ("ggr_epipolar_backward", ("valid", "segment", "dL_dfeatures", "dL_dimages"))])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    lib = _lib.load()
    fn = getattr(lib, entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -264, ctypes.sizeof(_lib.GgrEpipolarPass) - 4):
        ep = _pass()
        ep.struct_size = struct_size
        assert fn(ctypes.byref(ep), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrEpipolarPass" in _lib.last_error()


def test_an_empty_call_needs_no_gpu_and_the_scratch_size_query():
    lib = _lib.load()
    nothing = {f: None for f in POINTERS}
    assert lib.ggr_epipolar_forward(ctypes.byref(_pass(batch=0, scratch_bytes=0, **nothing)), None) == 0
    assert lib.ggr_epipolar_backward(ctypes.byref(_pass(batch=0, scratch_bytes=0, **nothing)), None) == 0
    assert lib.ggr_epipolar_forward(ctypes.byref(_pass(batch=0, num_samples=65, **nothing)), None) == GGR_E_INVALID   # (scalars still checked)
    assert lib.ggr_epipolar_scratch_bytes(1, 2, 128, 120, 88) == 2 * 128 * 120 * 88 * 4
    assert lib.ggr_epipolar_scratch_bytes(0, 2, 128, 120, 88) == 0
    for bad in ((1, 1, 128, 120, 88), (1, 9, 4, 4, 4), (1, 2, 513, 4, 4), (1, 2, 0, 4, 4), (1, 2, 4, 0, 4), (-1, 2, 4, 4, 4), (8192, 8, 4, 4, 4)):
        assert lib.ggr_epipolar_scratch_bytes(*bad) == -1, bad
