"""`fused_depth_head → fused_gaussian_adapter → render_cuda`, forward and backward, with ONE `to_gaussians` tensor feeding both
passes through its strided views `rows[..., :2]` and `rows[..., 2:]`.

  route A   the depth-head kernels, then the adapter kernels and the rasterizer
  route B   the same chain with the depth head replaced by its float32 torch restatement (tests/depth_head_reference.py) on the
            device, given the same uniform numbers
  chain64   the whole chain restated in float64 on the CPU: depth_head_reference → adapter_reference → `render_cuda` served by
            the torch oracle (oracle/torch_raster.py) instead of the HIP rasterizer

Route A must choose the same `index` as route B (and as chain64: the inputs obey the index-margin rule).  The image and the
gradients w.r.t. `logits` and the `to_gaussians` rows are held to the adapter's rule over route B's own float32 error:
e_A <= max(4·e_B, 1e-6) with e = max|x − chain64| / max|chain64|.  Adapter and rasterizer are float32 kernels in both routes,
so both errors carry theirs; the bar asks that the depth-head kernels add nothing beyond what the torch depth head adds.

2 context cameras × 16×12 rays, s = 32, one surface, d_sh = 25, one 48×32 target view; sampled with spp = 3 (plain form,
exponent 2**0.5) and deterministic with spp = 1 (transmittance form, exponent 1), as EncoderEpipolar.forward calls it."""
import math

import pytest
import torch

from oracle import torch_raster as tr
from tests.adapter_reference import adapter_reference, random_sh_transform
from tests.depth_head_reference import depth_head_reference, make_case

pytestmark = pytest.mark.gpu

RH, RW, S, D_SH = 12, 16, 32, 25
DEV = "cuda:0"


class _OracleRasterizer(torch.nn.Module):
    """TEST-ONLY stand-in for the HIP rasterizer (the torch oracle, any dtype, autograd on): chain64's last step"""

    def __init__(self, rs):
        super().__init__()
        self.rs = rs

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        rs = self.rs
        return tr.rasterize(means3D, opacities, rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg, rs.image_width, rs.image_height,
                            rs.tanfovx, rs.tanfovy, rs.sh_degree, shs=shs, colors_precomp=colors_precomp, cov3D_precomp=cov3D_precomp,
                            scales=scales, rotations=rotations, sh_cap=int(getattr(rs, "sh_max_degree", 0) or 3))


def _scene(mode, spp, transmittance, exponent):
    """float64 CPU leaves and settings of one chain"""
    g = torch.Generator().manual_seed(21)
    case = make_case(2, RH * RW, S, 1, spp, mode, seed=31, use_transmittance=transmittance, opacity_exponent=exponent,
                     image_shape=(RH, RW))
    case["near"], case["far"] = torch.tensor([2.0, 2.5], dtype=torch.float64), torch.tensor([8.0, 9.0], dtype=torch.float64)
    ys, xs = torch.meshgrid((torch.arange(RH, dtype=torch.float64) + 0.5) / RH, (torch.arange(RW, dtype=torch.float64) + 0.5) / RW,
                            indexing="ij")
    case["ray_xy"] = torch.stack([xs, ys], -1).reshape(-1, 2)
    del case["xy_raw"]
    rows = torch.randn(2, RH * RW, 2 + 7 + 3 * D_SH, generator=g, dtype=torch.float64).float().double()
    rows[..., 2:5] -= 2.0      # small splats
    rows[..., 9:] *= 3.0
    ext = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    a = 0.15
    ext[1, :3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float64)
    ext[:, :3, 3] = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.1, 0.1]], dtype=torch.float64)
    intr = torch.tensor([[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]], dtype=torch.float64).repeat(2, 1, 1)
    adapter = dict(extrinsics=ext, intrinsics=intr, sh_transform=random_sh_transform(2, D_SH, g, orthogonal=True).float().double())
    view = torch.eye(4, dtype=torch.float64)[None]
    view[..., :3, 3] = torch.tensor([0.1, 0.0, -0.5], dtype=torch.float64)
    target = dict(extrinsics=view, intrinsics=intr[:1].clone(), near=torch.tensor([1.0], dtype=torch.float64),
                  far=torch.tensor([100.0], dtype=torch.float64), background_color=torch.zeros(1, 3, dtype=torch.float64))
    upstream = torch.randn(1, 3, 32, 48, generator=g, dtype=torch.float64)
    return case, rows, adapter, target, upstream


def _chain(scene, head_fn, adapter_fn, dtype, device):
    """image, index and the gradients w.r.t. logits and rows of one route, as float64 CPU tensors"""
    from ggrt_official_amd import splatting as sp
    case, rows, adapter, target, upstream = scene
    to = lambda t: t.detach().clone().to(device=device, dtype=dtype) if torch.is_tensor(t) else t
    case, adapter = ({k: to(v) for k, v in d.items()} for d in (case, adapter))
    # the target camera is float32 in every route: the call site's camera setup is float32 by construction (get_fov,
    # get_projection_matrix), so all three chains see the same view and projection matrices
    target = {k: v.to(device=device, dtype=torch.float32) for k, v in target.items()}
    logits, rows = case.pop("logits").requires_grad_(True), to(rows).requires_grad_(True)
    head = head_fn(logits=logits, xy_raw=rows[..., :2], **case)
    head = head if isinstance(head, dict) else dict(depths=head.depths, opacities=head.opacities, coordinates=head.coordinates, index=head.index)
    out = adapter_fn(adapter["extrinsics"], adapter["intrinsics"], head["coordinates"], head["depths"], rows[..., 2:], (RH, RW),
                     adapter["sh_transform"], scale_min=0.5, scale_max=15.0)
    out = out if isinstance(out, dict) else dict(means=out.means, scales=out.scales, rotations=out.rotations, harmonics=out.harmonics)
    opacities = head["opacities"].reshape(1, -1)
    # the two passes share a layout: [C, G] is the decoder's [b, (v r srf spp)] without a copy
    assert opacities.data_ptr() == head["opacities"].data_ptr() and head["depths"].is_contiguous() and head["coordinates"].is_contiguous()
    img = sp.render_cuda(target["extrinsics"], target["intrinsics"], target["near"], target["far"], (32, 48), target["background_color"],
                         out["means"][None], None, out["harmonics"][None], opacities, gaussian_scales=out["scales"][None],
                         gaussian_rotations=out["rotations"][None])
    g_logits, g_rows = torch.autograd.grad((img * to(upstream)).sum(), [logits, rows])
    return dict(image=img.detach().double().cpu(), d_logits=g_logits.double().cpu(), d_rows=g_rows.double().cpu(),
                index=head["index"].detach().long().cpu())


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("mode,spp,transmittance,exponent", [("sampled", 3, False, 2 ** 0.5), ("deterministic", 1, True, 1.0)])
def test_depth_head_then_adapter_then_rasterizer_matches_the_torch_depth_head(monkeypatch, mode, spp, transmittance, exponent):
    from ggrt_official_amd import fused_depth_head, fused_gaussian_adapter
    from ggrt_official_amd import splatting as sp
    scene = _scene(mode, spp, transmittance, exponent)
    route_a = _chain(scene, fused_depth_head, fused_gaussian_adapter, torch.float32, DEV)
    route_b = _chain(scene, depth_head_reference, fused_gaussian_adapter, torch.float32, DEV)
    with monkeypatch.context() as m:
        m.setattr(sp, "GaussianRasterizer", _OracleRasterizer)
        chain64 = _chain(scene, depth_head_reference, adapter_reference, torch.float64, "cpu")
    assert torch.equal(route_a["index"], route_b["index"]) and torch.equal(route_a["index"], chain64["index"])
    assert route_a["image"].shape == (1, 3, 32, 48) and float(chain64["image"].abs().mean()) > 0.01
    # the rows' gradient arrives through both views: the depth head's two channels and the adapter's 82
    assert float(chain64["d_rows"][..., :2].abs().max()) > 0 and float(chain64["d_rows"][..., 2:].abs().max()) > 0
    bad = []
    for k in ("image", "d_logits", "d_rows"):
        e_a, e_b = _err(route_a[k], chain64[k]), _err(route_b[k], chain64[k])
        print(f"{mode} {k:9s} e_A {e_a:.3e}  e_B {e_b:.3e}  A against B {_err(route_a[k], route_b[k]):.3e}")
        if not (e_a <= max(4 * e_b, 1e-6)):
            bad.append((k, e_a, e_b))
    e_xy_a, e_xy_b = _err(route_a["d_rows"][..., :2], chain64["d_rows"][..., :2]), _err(route_b["d_rows"][..., :2], chain64["d_rows"][..., :2])
    print(f"{mode} d_rows[:2] e_A {e_xy_a:.3e}  e_B {e_xy_b:.3e}")
    if not (e_xy_a <= max(4 * e_xy_b, 1e-6)):
        bad.append(("d_rows[..., :2]", e_xy_a, e_xy_b))
    assert not bad, bad
