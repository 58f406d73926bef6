"""The image-loss pass (ggr_image_loss_forward / _backward, `fused_image_loss`, `fused_ssim`) — what needs no GPU: the symbols, the
layout of GgrImageLossPass against the compiled header, the refusal of every invalid pass before any GPU work, the library's 1-D
window against the reference's (bit for bit, from the fixtures), and the refusals of the Python entry points that come before any
launch."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
FIELDS = [f for f, _ in _lib.GgrImageLossPass._fields_]
SCALARS = ["struct_size", "reserved", "batch", "channels", "height", "width", "window_size", "size_average"]
POINTERS = ["pred", "target", "mask", "out_mse", "out_ssim", "mse_scale", "partials", "dL_dmse", "dL_dssim", "dL_dpred", "dL_dtarget"]
FORWARD = ("pred", "target", "out_mse", "out_ssim", "mse_scale", "partials")
BACKWARD = ("pred", "target", "mse_scale")
ENTRIES = ("ggr_image_loss_forward", "ggr_image_loss_backward")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES + ("ggr_image_loss_window", "ggr_image_loss_partials_bytes"):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    import ggrt_official_amd
    for name in ("fused_image_loss", "fused_ssim", "ImageLoss"):
        assert callable(getattr(ggrt_official_amd, name)) and name in ggrt_official_amd.__all__


def test_image_loss_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrEpipolarAttnEncPass", "GgrEpipolarAttnPass", "GgrEpipolarPass", "GgrDepthHeadPass", "GgrAdapterPass", "GgrSettings", "GgrViews")
    assert FIELDS == SCALARS + POINTERS[:7] + ["partials_bytes"] + POINTERS[7:]
    src = tmp_path / "il.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrImageLossPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrImageLossPass, {f}));\n' for f in FIELDS) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "il"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrImageLossPass) == size == 128
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(FIELDS)]:
        f, off = line.split()
        assert getattr(_lib.GgrImageLossPass, f).offset == int(off), f
    for line in lines[2 + len(FIELDS):2 + len(FIELDS) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrEpipolarAttnPass) == 88 and ctypes.sizeof(_lib.GgrEpipolarPass) == 264      # (as they were)
    assert _lib.image_loss_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, batch=2, channels=3, height=20, width=40, window_size=11, size_average=1, partials_bytes=1 << 20,
                **{f: 256 for f in POINTERS})
    base.update(kw)
    return _lib.image_loss_pass(**base)


BAD = [(dict(batch=0), ".batch "), (dict(batch=-1), ".batch "), (dict(channels=0), ".channels "), (dict(height=0), ".height "),
       (dict(width=0), ".width "), (dict(height=(1 << 20) + 1), ".height "), (dict(width=(1 << 20) + 1), ".width "),
       (dict(batch=1 << 20, channels=1 << 12), "tiles"), (dict(window_size=0), ".window_size "), (dict(window_size=4), ".window_size "),
       (dict(window_size=13), ".window_size "), (dict(window_size=-3), ".window_size "), (dict(size_average=2), ".size_average "),
       (dict(reserved=1), "reserved"), (dict(pred=258), "misaligned"), (dict(target=257), "misaligned"), (dict(mask=259), "misaligned"),
       (dict(mse_scale=262), "misaligned")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrImageLossPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_image_loss_forward", FORWARD), ("ggr_image_loss_backward", BACKWARD)])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    lib = _lib.load()
    fn = getattr(lib, entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -128, ctypes.sizeof(_lib.GgrImageLossPass) - 4):
        lp = _pass()
        lp.struct_size = struct_size
        assert fn(ctypes.byref(lp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrImageLossPass" in _lib.last_error()


def test_the_forward_checks_its_scratch_and_the_backward_needs_a_gradient_each_way():
    lib = _lib.load()
    need = lib.ggr_image_loss_partials_bytes(2, 3, 20, 40)
    assert need == 2 * 3 * 2 * 2 * 24                    # 16 x 32 tiles, three doubles each
    assert lib.ggr_image_loss_partials_bytes(1, 1, 16, 32) == 24 and lib.ggr_image_loss_partials_bytes(1, 1, 17, 33) == 4 * 24
    assert lib.ggr_image_loss_partials_bytes(0, 3, 20, 40) == -1 and lib.ggr_image_loss_partials_bytes(1, 1, 1 << 21, 4) == -1
    assert lib.ggr_image_loss_forward(ctypes.byref(_pass(partials_bytes=need - 8)), None) == GGR_E_INVALID and "partials_bytes" in _lib.last_error()
    assert lib.ggr_image_loss_forward(ctypes.byref(_pass(partials=260)), None) == GGR_E_INVALID and "partials" in _lib.last_error()
    assert lib.ggr_image_loss_backward(ctypes.byref(_pass(dL_dmse=None, dL_dssim=None)), None) == GGR_E_INVALID and "dL_dmse" in _lib.last_error()
    assert lib.ggr_image_loss_backward(ctypes.byref(_pass(dL_dpred=None, dL_dtarget=None)), None) == GGR_E_INVALID and "dL_dpred" in _lib.last_error()


def test_the_library_window_is_the_reference_window_bit_for_bit():
    lib = _lib.load()
    seen = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "image_loss_*.npz"))):
        z = np.load(path, allow_pickle=False)
        ws = int(z["window_size"])
        out = (ctypes.c_float * ws)()
        assert lib.ggr_image_loss_window(ws, out) == 0
        assert z["window"].dtype == np.float32 and np.array_equal(np.frombuffer(out, dtype=np.float32), z["window"]), path
        seen.add(ws)
    assert seen == {7, 11}
    from tests.image_loss_reference import gaussian       # the restatement builds the other sizes the same way
    for ws in (1, 3, 5, 7, 9, 11):
        out = (ctypes.c_float * ws)()
        assert lib.ggr_image_loss_window(ws, out) == 0
        assert np.array_equal(np.frombuffer(out, dtype=np.float32), gaussian(ws).numpy()), ws
    for ws in (0, 2, 12, 13, -1):
        assert lib.ggr_image_loss_window(ws, (ctypes.c_float * 16)()) == GGR_E_INVALID and "window_size" in _lib.last_error()
    assert lib.ggr_image_loss_window(11, None) == GGR_E_INVALID


def test_python_entry_points_refuse_before_any_launch():
    import torch
    from ggrt_official_amd import ImageLoss, fused_image_loss, fused_ssim
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="pred.*GPU only"):
        fused_image_loss(x, x)
    with pytest.raises(RuntimeError, match="pred.*GPU only"):
        fused_ssim(x, x)
    loss = ImageLoss(mse=torch.tensor(0.01), ssim=torch.tensor(0.9))
    assert abs(float(loss.psnr) + 10 * np.log10(0.01 + 1e-6)) < 1e-5 and tuple(loss) == (loss.mse, loss.ssim)
