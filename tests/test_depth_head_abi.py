"""The depth-head pass (ggr_depth_head_forward / ggr_depth_head_backward, `fused_depth_head`) — what needs no GPU: the symbols,
the layout of GgrDepthHeadPass against the compiled header, and the refusal of every invalid pass before any GPU work."""
import ctypes
import os
import subprocess

import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID, GGR_E_LIMIT = 1, 4
FIELDS = [f for f, _ in _lib.GgrDepthHeadPass._fields_] if hasattr(_lib, "GgrDepthHeadPass") else []
INPUTS = ("logits", "xy_raw", "ray_xy", "near", "far", "u")
OUTPUTS = ("out_depth", "out_opacity", "out_coords", "index")
GRADS_IN = ("dL_ddepth", "dL_dopacity", "dL_dcoords")
GRADS_OUT = ("dL_dlogits", "dL_dxy_raw")
ENTRIES = ("ggr_depth_head_forward", "ggr_depth_head_backward")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES:
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob


def test_depth_head_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrAdapterPass", "GgrProjectionPass", "GgrHitPass", "GgrHitGradPass", "GgrPickPass", "GgrContributionPass",
              "GgrFeaturePass", "GgrDistortionPass", "GgrAbsgradPass", "GgrSettings", "GgrViews", "GgrForwardIn", "GgrForwardOut",
              "GgrBackwardIn", "GgrBackwardOut")
    assert FIELDS[:2] == ["struct_size", "reserved"] and set(INPUTS + OUTPUTS + GRADS_IN + GRADS_OUT) < set(FIELDS)
    src = tmp_path / "dp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrDepthHeadPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrDepthHeadPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "dp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrDepthHeadPass) == size == 184
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrDepthHeadPass, f).offset == int(off), f
    for line in lines[2 + len(FIELDS):2 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrAdapterPass) == 248 and ctypes.sizeof(_lib.GgrProjectionPass) == 128   # (as they were)
    assert _lib.depth_head_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, num_cameras=2, rays_per_camera=12, num_buckets=32, num_surfaces=1, samples_per_ray=3, deterministic=0,
                use_transmittance=0, xy_raw_stride=2, debug=0, reserved2=0, opacity_exponent=1.0, opacity_scale=1.0 / 3, inv_w=1.0 / 24,
                inv_h=1.0 / 16, **{f: 256 for f in INPUTS + OUTPUTS + GRADS_IN + GRADS_OUT})
    base.update(kw)
    return _lib.depth_head_pass(**base)


BAD = [(dict(num_buckets=0), GGR_E_INVALID, "num_buckets"), (dict(num_buckets=65), GGR_E_LIMIT, "num_buckets"),
       (dict(samples_per_ray=0), GGR_E_INVALID, "samples_per_ray"), (dict(samples_per_ray=17), GGR_E_LIMIT, "samples_per_ray"),
       (dict(deterministic=1, num_buckets=2), GGR_E_INVALID, "samples_per_ray"),
       (dict(num_surfaces=0), GGR_E_INVALID, "num_surfaces"), (dict(num_surfaces=-2), GGR_E_INVALID, "num_surfaces"),
       (dict(num_cameras=65536), GGR_E_LIMIT, "num_cameras"),
       (dict(num_cameras=60000, rays_per_camera=60000), GGR_E_LIMIT, "too large"),
       (dict(rays_per_camera=1 << 20, num_surfaces=1 << 10), GGR_E_LIMIT, "too large"),
       (dict(reserved=1), GGR_E_INVALID, "reserved"), (dict(reserved2=7), GGR_E_INVALID, "reserved"),
       (dict(num_cameras=-1), GGR_E_INVALID, "negative"), (dict(rays_per_camera=-3), GGR_E_INVALID, "negative"),
       (dict(xy_raw_stride=1), GGR_E_INVALID, "xy_raw_stride"), (dict(xy_raw_stride=0), GGR_E_INVALID, "xy_raw_stride"),
       (dict(logits=258), GGR_E_INVALID, "misaligned"), (dict(index=257), GGR_E_INVALID, "misaligned"),
       (dict(dL_dxy_raw=259), GGR_E_INVALID, "misaligned"),
       (dict(logits=None), GGR_E_INVALID, "logits"), (dict(xy_raw=None), GGR_E_INVALID, "xy_raw"),
       (dict(ray_xy=None), GGR_E_INVALID, "ray_xy"), (dict(near=None), GGR_E_INVALID, "near"), (dict(far=None), GGR_E_INVALID, "far")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,code,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, code, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == code and msg in _lib.last_error() and "GgrDepthHeadPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_depth_head_forward", OUTPUTS + ("u",)), ("ggr_depth_head_backward", ("index", "dL_dlogits"))])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    lib = _lib.load()
    fn = getattr(lib, entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -184, ctypes.sizeof(_lib.GgrDepthHeadPass) - 4):
        dp = _pass()
        dp.struct_size = struct_size
        assert fn(ctypes.byref(dp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrDepthHeadPass" in _lib.last_error()


def test_what_may_be_null_is_not_asked_for_and_an_empty_call_needs_no_gpu():
    """C = 0 or R = 0 is valid and enqueues nothing: GGR_OK in a process without a GPU, with every pointer NULL"""
    lib = _lib.load()
    nothing = {f: None for f in INPUTS + OUTPUTS + GRADS_IN + GRADS_OUT}
    for dims in (dict(num_cameras=0), dict(rays_per_camera=0)):
        for det in (0, 1):
            assert lib.ggr_depth_head_forward(ctypes.byref(_pass(deterministic=det, **dims, **nothing)), None) == 0
            assert lib.ggr_depth_head_backward(ctypes.byref(_pass(deterministic=det, **dims, **nothing)), None) == 0
    # the scalars of an empty call are still checked
    assert lib.ggr_depth_head_forward(ctypes.byref(_pass(num_cameras=0, num_buckets=65, **nothing)), None) == GGR_E_LIMIT
