"""The contribution pass (ggr_contributions, `return_contributions`) — what needs no GPU: the symbol, the layout of
GgrContributionPass against the compiled header, the refusal of every invalid pass before any GPU work, and the call surface."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = ("struct_size", "reserved", "geom_buffer", "image_buffer", "binning_buffer", "num_rendered", "out_weight_sum",
          "out_weight_max", "out_pixel_count")


def test_symbol_exists_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.ggr_contributions is not None and "ggr_contributions" in [s[0] for s in _lib.SYMBOLS]


def test_contribution_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrFeaturePass", "GgrForwardExtra", "GgrBackwardExtra", "GgrForwardOptions", "GgrSettings", "GgrViews",
              "GgrForwardIn", "GgrForwardOut", "GgrBackwardIn", "GgrBackwardOut")
    src = tmp_path / "cp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(GgrContributionPass));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrContributionPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "cp"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrContributionPass) == size == 64
    assert [f for f, _ in _lib.GgrContributionPass._fields_] == list(FIELDS)
    for line in lines[1:1 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrContributionPass, f).offset == int(off), f
    for line in lines[1 + len(FIELDS):1 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert _lib.contribution_pass().struct_size == size


def _pass(**kw):
    base = dict(geom_buffer=256, image_buffer=256, binning_buffer=256, num_rendered=1, out_weight_sum=256, out_weight_max=256,
                out_pixel_count=256)
    base.update(kw)
    return _lib.contribution_pass(**base)


def _settings():
    return _lib.GgrSettings(image_height=32, image_width=48, num_points=10)


BAD = [
    (dict(reserved=1), "reserved"),
    (dict(out_weight_sum=None, out_weight_max=None, out_pixel_count=None), "every output is NULL"),
    (dict(geom_buffer=None), "geom"),
    (dict(image_buffer=None), "geom"),
    (dict(binning_buffer=None), "binning_buffer"),
]


@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return GGR_E_INVALID with this text)"""
    lib = _lib.load()
    st = _settings()
    rc = lib.ggr_contributions(ctypes.byref(st), None, ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("struct_size", [0, 8, -64, ctypes.sizeof(_lib.GgrContributionPass) - 4])
def test_bad_struct_size_is_refused(struct_size):
    lib = _lib.load()
    cp = _pass()
    cp.struct_size = struct_size
    st = _settings()
    assert lib.ggr_contributions(ctypes.byref(st), None, ctypes.byref(cp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert lib.ggr_contributions(ctypes.byref(st), None, None, None) == GGR_E_INVALID
    vw = _lib.GgrViews(num_views=3, num_sets=2)
    assert lib.ggr_contributions(ctypes.byref(st), ctypes.byref(vw), ctypes.byref(_pass()), None) == GGR_E_INVALID
    assert "num_sets" in _lib.last_error()


def test_call_surface():
    import ggrt_official_amd as g
    from ggrt_official_amd import splatting as S
    # the settings: the tuple's fields are what they were; the new setting rides behind them (keyword, or positional last)
    S0 = g.GaussianRasterizationSettings
    assert S0._fields[-1] == "return_alpha" and "return_contributions" not in S0._fields
    e = torch.eye(4)
    kw = dict(image_height=32, image_width=48, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=e,
              projmatrix=e, sh_degree=3, campos=torch.zeros(3), prefiltered=False)
    off, on = S0(**kw), S0(**kw, return_contributions=True)
    assert off.return_contributions is False and on.return_contributions is True and len(on) == len(off) == len(S0._fields)
    assert on._replace(sh_max_degree=4).return_contributions is True and on._replace(sh_max_degree=4).sh_max_degree == 4
    assert off._replace(return_contributions=True).return_contributions is True and off.return_contributions is False
    assert on._replace(return_contributions=False, return_alpha=True).return_contributions is False
    assert S0(*off, True).return_contributions is True and S0(*off).return_contributions is False       # positional, last
    assert isinstance(on._replace(debug=True), S0) and on._asdict()["return_contributions"] is True
    assert S0._make(list(on)).return_contributions is False
    import copy, pickle
    assert copy.copy(on).return_contributions is True and pickle.loads(pickle.dumps(on)).return_contributions is True
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw, return_contributions=True))._settings_for_call().return_contributions is True
    assert g.Contributions._fields == ("weight_sum", "weight_max", "pixel_count") and S.Contributions is g.Contributions
    for fn in (S.render_cuda, S.render_color_and_depth, S.render_views_fused, S.DecoderSplattingCUDA.forward,
               S.boundary_arguments):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "return_contributions" and p["return_contributions"].default is False, fn
    c, d = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert S.DecoderOutput(c, d).contributions is None and S.DecoderOutput(c, d, d, c).contributions is None
    assert S._fused_result(c, d, None, False) == (c, d) and S._fused_result(c, d, None, False, c)[-1] is c   # as before
    assert S._fused_result(c, d, None, False, c, "x") == (c, d, c, "x")
    assert "contribution_keep_mask" in dir(S) and "return_contributions" not in inspect.signature(S.DecoderSplattingCUDA.__init__).parameters
