"""`DecoderSplattingCUDA → fused_image_loss`, forward and backward: the training step's tail, 0.8·mse + 0.2·(1 − ssim) of the
rendered views against a target with a mask, back-propagated to the Gaussians.

  route A   the decoder's render, then the image-loss kernels
  route B   the same render, then the float32 torch restatement of the reference's two functions (tests/image_loss_reference.py)
            on the device
  ref       the same render, then the restatement in float64 on the CPU; its dL/dimage, rounded to float32 once, goes through the
            same rasterizer backward

The rasterizer is the same float32 kernel in all three, so what differs is dL/dimage alone.  The Gaussians' gradients are held to
the other call-site tests' rule over route B's own error: e_A <= max(4·e_B, 1e-6) with e = max|x − ref| / max|ref|.

1 batch × 2 views of 64 × 96 pixels (two by three tiles of the loss kernel each way), 2000 Gaussians with 9 SH coefficients."""
import pytest
import torch

from tests.image_loss_reference import image_loss_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("means", "covariances", "harmonics", "opacities")


def _scene():
    gen = torch.Generator().manual_seed(1301)
    b, v, n, d_sh, h, w = 1, 2, 2000, 9, 64, 96
    ext = torch.eye(4).repeat(b, v, 1, 1)
    ext[..., 0, 3] = torch.linspace(-0.2, 0.2, v)
    K = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    means = torch.randn(b, n, 3, generator=gen) * torch.tensor([0.6, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(b, n, 3, 3, generator=gen) * 0.05
    cov = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3)
    harm = torch.randn(b, n, 3, d_sh, generator=gen) * 0.3
    opac = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    noise = 0.1 * torch.randn(v, 3, h, w, generator=gen)
    mask = 0.5 * torch.randint(0, 3, (v, h, w), generator=gen).float()
    return (means, cov, harm, opac), (ext, K, near, far, (h, w)), noise, mask


def _route(loss_fn, leaves, cams):
    """the rendered views and the Gaussians' gradients of 0.8·mse + 0.2·(1 − ssim); loss_fn(image) -> the loss, or dL/dimage"""
    from ggrt_official_amd import splatting as S
    leaves = [t.detach().clone().to(DEV).requires_grad_(True) for t in leaves]
    dec = S.DecoderSplattingCUDA(sh_max_degree=3).to(DEV)
    ext, K, near, far, shape = cams
    image = dec(S.Gaussians(*leaves), ext.to(DEV), K.to(DEV), near.to(DEV), far.to(DEV), shape).color.flatten(0, 1)
    out = loss_fn(image)
    if out.shape == image.shape:      # ref: dL/dimage computed elsewhere
        grads = torch.autograd.grad(image, leaves, out)
    else:
        grads = torch.autograd.grad(out, leaves)
    return image.detach(), dict(zip(NAMES, (g.double().cpu() for g in grads)))


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def test_render_then_fused_loss_matches_render_then_torch_loss():
    from ggrt_official_amd import fused_image_loss
    leaves, cams, noise, mask = _scene()
    mix = lambda mse, ssim: 0.8 * mse + 0.2 * (1 - ssim)

    # the target: the render itself plus noise, clamped — fixed before the routes, the same tensor in all of them
    from ggrt_official_amd import splatting as S
    with torch.no_grad():
        ext, K, near, far, shape = cams
        dec = S.DecoderSplattingCUDA(sh_max_degree=3).to(DEV)
        image0 = dec(S.Gaussians(*(t.to(DEV) for t in leaves)), ext.to(DEV), K.to(DEV), near.to(DEV), far.to(DEV), shape).color.flatten(0, 1)
    target = (image0 + noise.to(DEV)).clamp(0, 1)
    mask_d = mask.to(DEV)

    def fused(image):
        out = fused_image_loss(image, target, mask_d)
        return mix(out.mse, out.ssim)

    def torch32(image):
        return mix(*image_loss_reference(image, target, mask_d))

    def float64(image):
        x = image.detach().double().cpu().requires_grad_(True)
        (g,) = torch.autograd.grad(mix(*image_loss_reference(x, target.double().cpu(), mask.double())), [x])
        return g.float().to(DEV)

    img_a, a = _route(fused, leaves, cams)
    img_b, b = _route(torch32, leaves, cams)
    img_r, ref = _route(float64, leaves, cams)
    assert torch.equal(img_a, image0) and torch.equal(img_b, image0) and torch.equal(img_r, image0)
    assert img_a.shape == (2, 3, 64, 96) and float(img_a.mean()) > 0.01
    bad = []
    for k in NAMES:
        assert float(ref[k].abs().max()) > 0, k
        e_a, e_b = _err(a[k], ref[k]), _err(b[k], ref[k])
        print(f"{k:12s} e_A {e_a:.3e}  e_B {e_b:.3e}  A against B {_err(a[k], b[k]):.3e}")
        if not (e_a <= max(4 * e_b, 1e-6)):
            bad.append((k, e_a, e_b))
    assert not bad, bad
