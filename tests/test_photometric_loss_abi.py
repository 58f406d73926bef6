"""The photometric-loss pass (ggr_photometric_loss_forward / _backward, `fused_photometric_loss`) — what needs no GPU: the symbols,
the layout of GgrPhotometricLossPass against the compiled header, the ABI version, the refusal of every invalid pass before any GPU
work, the size queries, and the refusals of the Python entry point, each naming the torch route."""
import ctypes
import os
import subprocess

import pytest
import torch

from ggrt_official_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GGR_E_INVALID = 1
ENTRIES = ("ggr_photometric_loss_forward", "ggr_photometric_loss_backward")
COMMON = ("image", "ref_imgs", "inv_depths", "K", "ref_Ks", "poses", "planes", "workspace", "out_thresholds", "state", "choice")
FORWARD = COMMON + ("out_loss", "out_photometric", "out_smoothness")
BACKWARD = COMMON + ("dL_dloss", "dL_dinv_depths", "dL_dposes")


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ggr_abi_version() == _lib.ABI_VERSION == 11
    names = [s[0] for s in _lib.SYMBOLS]
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for sym in ENTRIES + ("ggr_photometric_loss_planes_bytes", "ggr_photometric_loss_workspace_bytes"):
        assert getattr(lib, sym) is not None and sym in names and sym.encode() in blob
    import ggrt_official_amd
    for name in ("fused_photometric_loss", "PhotometricLoss"):
        assert callable(getattr(ggrt_official_amd, name)) and name in ggrt_official_amd.__all__


def test_pass_layout_matches_header_and_no_other_struct_grew(tmp_path):
    others = ("GgrImageLossPass", "GgrEpipolarAttnEncPass", "GgrEpipolarAttnPass", "GgrEpipolarPass", "GgrDepthHeadPass", "GgrAdapterPass", "GgrSettings", "GgrViews")
    fields = [f for f, _ in _lib.GgrPhotometricLossPass._fields_]
    src = tmp_path / "pl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggr_raster.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(GgrPhotometricLossPass), (int)GGR_ABI_VERSION);\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(GgrPhotometricLossPass, {f}));\n' for f in fields) +
                   "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in others) + "  return 0;\n}\n")
    exe = tmp_path / "pl"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size = int(lines[0])
    assert ctypes.sizeof(_lib.GgrPhotometricLossPass) == size == 208
    assert int(lines[1]) == _lib.ABI_VERSION == 11
    for line in lines[2:2 + len(fields)]:
        f, off = line.split()
        assert getattr(_lib.GgrPhotometricLossPass, f).offset == int(off), f
    for line in lines[2 + len(fields):2 + len(fields) + len(others)]:
        s, n = line.split()
        assert ctypes.sizeof(getattr(_lib, s)) == int(n), s
    assert ctypes.sizeof(_lib.GgrImageLossPass) == 128            # (as it was)
    assert _lib.photometric_loss_pass().struct_size == size


def _pass(**kw):
    base = dict(reserved=0, num_views=2, num_iters=3, height=20, width=40, automask=1, reserved2=0, ssim_loss_weight=0.85, smooth_loss_weight=0.01,
                C1=1e-4, C2=9e-4, clip_loss=0.5, gamma=0.85, planes_bytes=1 << 24, workspace_bytes=1 << 24,
                **{f: 256 for f in set(FORWARD + BACKWARD)})
    base.update(kw)
    return _lib.photometric_loss_pass(**base)


BAD = [(dict(num_views=0), ".num_views "), (dict(num_views=-1), ".num_views "), (dict(num_iters=0), ".num_iters "), (dict(num_iters=1025), ".num_iters "),
       (dict(height=1), ".height "), (dict(width=1), ".width "), (dict(height=16385), ".height "), (dict(width=16385), ".width "),
       (dict(automask=2), ".automask "), (dict(num_views=9), "candidates"), (dict(num_views=17, automask=0), "candidates"),
       (dict(ssim_loss_weight=0.0), ".ssim_loss_weight "), (dict(ssim_loss_weight=-0.5), ".ssim_loss_weight "), (dict(ssim_loss_weight=1.5), ".ssim_loss_weight "),
       (dict(ssim_loss_weight=float("nan")), ".ssim_loss_weight "), (dict(smooth_loss_weight=-1.0), ".smooth_loss_weight "),
       (dict(clip_loss=-0.1), ".clip_loss "), (dict(gamma=float("inf")), ".gamma "), (dict(C2=float("nan")), ".C2 "),
       (dict(reserved=1), "reserved"), (dict(reserved2=1), "reserved"), (dict(image=258), "misaligned"), (dict(poses=257), "misaligned"),
       (dict(workspace=260), "workspace is misaligned"), (dict(planes_bytes=1024), "planes_bytes"), (dict(workspace_bytes=64), "workspace_bytes")]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fields,msg", BAD)
def test_invalid_passes_are_refused_before_any_gpu_work(entry, fields, msg):
    """(no GPU in this process: a call that got as far as enqueueing anything could not return this code with this text)"""
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(_pass(**fields)), None)
    assert rc == GGR_E_INVALID and msg in _lib.last_error() and "GgrPhotometricLossPass" in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("entry,fields", [("ggr_photometric_loss_forward", FORWARD), ("ggr_photometric_loss_backward", BACKWARD)])
def test_null_required_pointers_and_bad_struct_sizes_are_refused(entry, fields):
    fn = getattr(_lib.load(), entry)
    for f in fields:
        assert fn(ctypes.byref(_pass(**{f: None})), None) == GGR_E_INVALID and f in _lib.last_error(), f
    for struct_size in (0, 8, -128, ctypes.sizeof(_lib.GgrPhotometricLossPass) - 4):
        lp = _pass()
        lp.struct_size = struct_size
        assert fn(ctypes.byref(lp), None) == GGR_E_INVALID and "struct_size" in _lib.last_error()
    assert fn(None, None) == GGR_E_INVALID and "GgrPhotometricLossPass" in _lib.last_error()


def test_the_size_queries():
    lib = _lib.load()
    assert lib.ggr_photometric_loss_planes_bytes(5, 13, 378, 504, 1) == (13 * 5 + 5) * 378 * 504 * 4
    assert lib.ggr_photometric_loss_planes_bytes(5, 13, 378, 504, 0) == 13 * 5 * 378 * 504 * 4
    tiles = 24 * 16
    assert lib.ggr_photometric_loss_workspace_bytes(5, 13, 378, 504, 1) == max((70 * 3 + 13 * 3) * tiles, tiles * 13 * 5 * 12) * 8
    assert lib.ggr_photometric_loss_workspace_bytes(8, 1, 16, 32, 1) > 0 and lib.ggr_photometric_loss_workspace_bytes(9, 1, 16, 32, 1) == -1
    assert lib.ggr_photometric_loss_planes_bytes(1, 1, 1, 32, 1) == -1 and lib.ggr_photometric_loss_planes_bytes(1, 1, 2, 2, 2) == -1


def test_python_entry_point_refuses_before_any_launch():
    from ggrt_official_amd import fused_photometric_loss
    V, n, H, W = 2, 2, 8, 12
    img, refs, inv = torch.zeros(1, 3, H, W), torch.zeros(V, 3, H, W), torch.ones(n, 1, H, W)
    K, Ks, poses = torch.eye(3)[None], torch.eye(3).repeat(V, 1, 1), torch.zeros(V, n, 6)
    with pytest.raises(RuntimeError, match="image.*GPU only"):
        fused_photometric_loss(img, refs, inv, K, Ks, poses)
    route = "MultiViewPhotometricDecayLoss"
    with pytest.raises(ValueError, match="padding_mode.*" + route):
        fused_photometric_loss(img, refs, inv, K, Ks, poses, padding_mode="border")
    with pytest.raises(ValueError, match="photometric_reduce_op.*" + route):
        fused_photometric_loss(img, refs, inv, K, Ks, poses, photometric_reduce_op="mean")
    with pytest.raises(ValueError, match="V·n = 0.*" + route):
        fused_photometric_loss(img, refs, [], K, Ks, poses)
    with pytest.raises(ValueError, match="batch other than 1.*" + route):
        fused_photometric_loss(img, refs, [torch.ones(2, 1, H, W)], K, Ks, poses)
    with pytest.raises(ValueError, match="one resolution.*" + route):
        fused_photometric_loss(img, refs, [torch.ones(1, 1, H, W), torch.ones(1, 1, H // 2, W // 2)], K, Ks, poses)


@pytest.mark.gpu
def test_python_entry_point_refuses_the_forms_it_does_not_take_on_the_device():
    from ggrt_official_amd import fused_photometric_loss
    dev = "cuda"
    V, n, H, W = 2, 2, 8, 12
    mk = lambda V=V, n=n, H=H, W=W, B=1: (torch.zeros(B, 3, H, W, device=dev), torch.zeros(V, 3, H, W, device=dev), torch.ones(n, 1, H, W, device=dev),
                                          torch.eye(3, device=dev)[None], torch.eye(3, device=dev).repeat(V, 1, 1), torch.zeros(V, n, 6, device=dev))
    route = "MultiViewPhotometricDecayLoss"
    with pytest.raises(ValueError, match="batch other than 1.*" + route):
        fused_photometric_loss(*mk(B=2))
    a = list(mk())
    a[2] = torch.ones(n, 1, H // 2, W // 2, device=dev)
    with pytest.raises(ValueError, match="resolution.*" + route):
        fused_photometric_loss(*a)
    with pytest.raises(ValueError, match="ssim_loss_weight.*" + route):
        fused_photometric_loss(*mk(), ssim_loss_weight=0.0)
    with pytest.raises(ValueError, match="below 2 x 2.*" + route):
        fused_photometric_loss(*mk(H=1))
    with pytest.raises(ValueError, match="V·n = 0.*" + route):
        fused_photometric_loss(*mk(V=0))
    with pytest.raises(ValueError, match="candidates.*" + route):
        fused_photometric_loss(*mk(V=9))
    assert fused_photometric_loss(*mk(V=8)).loss.shape == (1,)          # the cap covers V = 8 with the auto-mask
    with pytest.raises(RuntimeError, match="ref_imgs requires grad"):
        a = list(mk())
        a[1].requires_grad_(True)
        fused_photometric_loss(*a)
