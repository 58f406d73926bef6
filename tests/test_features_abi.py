"""The feature pass (ggr_features_forward / ggr_features_backward, `features_precomp`) — what needs no GPU: the symbols, the
layout of GgrFeaturePass against the compiled header, the pinned sizes of the extra structs, the refusal of every invalid pass
before any GPU work, and the call surface."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "num_features", "features", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered",
          "out_features", "dL_dout_features", "dL_dfeatures", "scratch", "scratch_zeroed", "reserved")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11
    for name in ("ggr_features_forward", "ggr_features_backward"):
        assert getattr(lib, name) is not None and name in [s[0] for s in _lib.SYMBOLS]


def test_feature_pass_layout_matches_header_and_the_extras_stay_16_bytes(tmp_path):
    src = tmp_path / "fp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d\\n", sizeof(GgrFeaturePass), sizeof(GgrForwardExtra), sizeof(GgrBackwardExtra), '
                   "GGR_MAX_FEATURES);\n" +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrFeaturePass, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "fp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size, fwd_extra, bwd_extra, kmax = (int(x) for x in lines[0].split())
    assert ctypes.sizeof(_lib.GgrFeaturePass) == size
    assert fwd_extra == bwd_extra == 16 == ctypes.sizeof(_lib.GgrForwardExtra) == ctypes.sizeof(_lib.GgrBackwardExtra)
    assert kmax == _lib.MAX_FEATURES == 32
    assert [f for f, _ in _lib.GgrFeaturePass._fields_] == list(FIELDS)
    for line in lines[1:1 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrFeaturePass, f).offset == int(off), f
    assert _lib.feature_pass(num_features=3).struct_size == size


def _pass(**kw):
    base = dict(num_features=4, features=256, geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1,
                out_features=256, dL_dout_features=256, dL_dfeatures=256, scratch=256)
    base.update(kw)
    return _lib.feature_pass(**base)


def _settings():
    return _lib.GgrSettings(image_height=32, image_width=48, num_points=10)


BAD = [
    (dict(num_features=0), "num_features", "both"),
    (dict(num_features=33), "num_features", "both"),
    (dict(num_features=-1), "num_features", "both"),
    (dict(reserved=1), "reserved", "both"),
    (dict(out_features=None), "out_features", "both"),
    (dict(features=None), "features", "both"),
    (dict(geom_buffer=None), "geom", "both"),
    (dict(image_buffer=None), "geom", "both"),
    (dict(binning_buffer=None), "binning_buffer", "both"),
    (dict(dL_dout_features=None), "dL_dout_features", "backward"),
    (dict(dL_dfeatures=None), "dL_dfeatures", "backward"),
    (dict(scratch=None), "scratch", "backward"),
]


@pytest.mark.parametrize("which,fields,msg", [(w, f, m) for f, m, a in BAD for w in ("forward", "backward")
                                              if a == "both" or w == a])
def test_invalid_passes_are_refused_before_any_gpu_work(which, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    fn = lib.ggr_features_forward if which == "forward" else lib.ggr_features_backward
    st = _settings()
    rc = fn(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("which", ["forward", "backward"])
@pytest.mark.parametrize("struct_size", [0, 8, -80, ctypes.sizeof(_lib.GgrFeaturePass) - 4])
def test_bad_struct_size_is_refused(which, struct_size):
    lib = _lib.load()
    fn = lib.ggr_features_forward if which == "forward" else lib.ggr_features_backward
    fp = _pass()
    fp.struct_size = struct_size
    st = _settings()
    assert fn(ctypes.byref(st), None, ctypes.byref(fp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert fn(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID and "num_sets" in _lib.last_error()


def test_call_surface_accepts_the_keyword():
    import diff_gaussian_rasterization as dgr
    import ggrt_official_amd as g
    from ggrt_official_amd import splatting as S
    for fn in (g.GaussianRasterizer.forward, g.rasterize_gaussians, g.rasterize_views, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "features_precomp" in p and p["features_precomp"].default is None, fn
    assert list(inspect.signature(g.rasterize_gaussians).parameters)[-1] == "features_precomp"   # appended: positional calls as before
    for fn in (S.render_cuda, S.render_color_and_depth, S.render_views_fused, S.DecoderSplattingCUDA.forward):
        p = inspect.signature(fn).parameters
        assert "gaussian_features" in p and p["gaussian_features"].default is None, fn
    c, d = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert S.DecoderOutput(c, d).features is None and S.DecoderOutput(c, d, d).features is None   # positional construction as before
    assert S.DecoderOutput(c, d, None, c).features is c
    assert S._fused_result(c, d, None, False) == (c, d) and len(S._fused_result(c, d, d, True)) == 3   # tuples unchanged without features
    assert S._fused_result(c, d, None, False, c)[-1] is c


def test_wrong_feature_shapes_are_refused_in_python():
    from ggrt_official_amd.rasterizer import _features_2d
    assert _features_2d(torch.zeros(10, 7, dtype=torch.float64), 10, "x").dtype == torch.float32
    for bad in (torch.zeros(10), torch.zeros(9, 4), torch.zeros(10, 0), torch.zeros(10, 33), torch.zeros(2, 5, 4)):
        with pytest.raises(RuntimeError, match="features_precomp"):
            _features_2d(bad, 10, "x")
