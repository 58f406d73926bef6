"""The distortion pass (ggr_distortion_forward / ggr_distortion_backward, `return_distortion`) — what needs no GPU: the symbols,
the layout of GgrDistortionPass against the compiled header, the refusal of every invalid pass before any GPU work, and the
setting's place beside the settings tuple."""
import copy
import ctypes
import os
import pickle
import subprocess

import pytest
import torch

import ggrt_official_amd as g
from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "reserved", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "out_distortion", "totals",
          "dL_dout_distortion", "scratch", "scratch_zeroed", "reserved2")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    names = [s[0] for s in _lib.SYMBOLS]
    assert lib.ggr_distortion_forward is not None and lib.ggr_distortion_backward is not None
    assert "ggr_distortion_forward" in names and "ggr_distortion_backward" in names


def test_distortion_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = {"GgrPickPass": 80, "GgrContributionPass": 64, "GgrForwardExtra": 16, "GgrBackwardExtra": 16}
    src = tmp_path / "dp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(GgrDistortionPass));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrDistortionPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "dp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrDistortionPass) == size == 80
    assert [f for f, _ in _lib.GgrDistortionPass._fields_] == list(FIELDS)
    for line in lines[1:1 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrDistortionPass, f).offset == int(off), f
    for line in lines[1 + len(FIELDS):1 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n) == others[s], s
    assert _lib.distortion_pass().struct_size == size


def _pass(**kw):
    base = dict(geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1, out_distortion=256, totals=256,
                dL_dout_distortion=256, scratch=256)
    base.update(kw)
    return _lib.distortion_pass(**base)


def _settings():
    return _lib.GgrSettings(image_height=32, image_width=48, num_points=10)


BAD = [
    ("both", dict(reserved=1), "reserved"),
    ("both", dict(reserved2=1), "reserved"),
    ("both", dict(out_distortion=None), "out_distortion"),
    ("both", dict(geom_buffer=None), "geom"),
    ("both", dict(image_buffer=None), "geom"),
    ("both", dict(binning_buffer=None), "binning_buffer"),
    ("backward", dict(totals=None), "totals"),
    ("backward", dict(dL_dout_distortion=None), "dL_dout_distortion"),
    ("backward", dict(scratch=None), "scratch"),
]


@pytest.mark.parametrize("which,fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(which, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    for fn in ([lib.ggr_distortion_forward] if which == "both" else []) + [lib.ggr_distortion_backward]:
        rc = fn(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
        assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrDistortionPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("which", ["ggr_distortion_forward", "ggr_distortion_backward"])
@pytest.mark.parametrize("struct_size", [0, 8, -80, ctypes.sizeof(_lib.GgrDistortionPass) - 4])
def test_bad_struct_size_is_refused(which, struct_size):
    lib = _lib.load()
    fn = getattr(lib, which)
    dp = _pass()
    dp.struct_size = struct_size
    st = _settings()
    assert fn(ctypes.byref(st), None, ctypes.byref(dp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert fn(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()


def test_return_distortion_rides_beside_the_settings_tuple():
    e = torch.eye(4)
    kw = dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=e,
              projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False)
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "return_distortion" not in S0._fields
    off, on = S0(**kw), S0(**kw, return_distortion=True)
    assert off.return_distortion is False and on.return_distortion is True
    assert on.return_contributions is False and on.return_picks is False
    assert len(on) == len(off) == len(S0._fields) and tuple(on)[:4] == tuple(off)[:4]
    assert on._replace(sh_max_degree=4).return_distortion is True and off._replace(return_distortion=True).return_distortion is True
    both = on._replace(return_picks=True)
    assert both.return_distortion is True and both.return_picks is True and both._replace(return_distortion=False).return_picks is True
    assert on._asdict()["return_distortion"] is True and list(on._asdict())[:len(S0._fields)] == list(S0._fields)
    assert "return_distortion=True" in repr(on) and "return_distortion=False" in repr(off)
    # keyword only: the positional slots behind the tuple's fields stay return_contributions, return_picks
    assert S0(*off, True, True).return_distortion is False
    with pytest.raises(TypeError):
        S0(*off, False, False, True)
    assert S0._make(list(on)).return_distortion is False
    assert copy.copy(on).return_distortion is True and pickle.loads(pickle.dumps(on)).return_distortion is True
