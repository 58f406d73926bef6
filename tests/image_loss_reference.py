"""A restatement in torch of the two functions `fused_image_loss` replaces — GGRt's `img2mse(x, y, mask)` (utils_loc.py:49-60) and
`ssim(img1, img2, window_size, size_average)` (ggrt/loss/ssim_torch.py) — for any dtype on any device, and the inputs the tests share.

`pred`, `target` are [B,C,H,W], `mask` [B,H,W] float weights or None.  The window is built as the reference builds it: the taps
in float32 from Python's `exp`, normalised in float32, the 2-D window their float32 outer product, and only then cast to the
images' dtype (`window.type_as(img1)`).  `separable=True` applies the 1-D window along rows and then columns instead of the 2-D one:
what the kernel does.  `img2mse` sees the channels-last view of the same data; with `size_average=False` every image gets its own
`img2mse` with its own mask slice and its own SSIM mean."""
from math import exp

import torch
import torch.nn.functional as F

TINY_NUMBER = 1e-6
C1, C2 = 0.01 ** 2, 0.03 ** 2
NOISES = (0.02, 0.1, 0.3)      # SSIM 0.998, 0.95-0.97 and 0.71 on make_image_case's images


def gaussian(window_size, sigma=1.5):
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return gauss / gauss.sum()


def _convolve(img, window_size, separable):
    """separable: False — the reference's 2-D window (float32 products of the taps); True — rows, then columns; "outer" — the 2-D
    window as the outer product of the taps in the images' dtype (what the separable route equals up to summation order)"""
    c = img.shape[1]
    w1 = gaussian(window_size).unsqueeze(1)
    pad = window_size // 2
    if separable == "outer":
        w = w1.to(device=img.device, dtype=img.dtype)
        return F.conv2d(img, (w @ w.t()).expand(c, 1, window_size, window_size).contiguous(), padding=pad, groups=c)
    if separable:
        w = w1.to(device=img.device, dtype=img.dtype)
        rows = F.conv2d(img, w.t().reshape(1, 1, 1, -1).expand(c, 1, 1, window_size).contiguous(), padding=(0, pad), groups=c)
        return F.conv2d(rows, w.reshape(1, 1, -1, 1).expand(c, 1, window_size, 1).contiguous(), padding=(pad, 0), groups=c)
    w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(c, 1, window_size, window_size).contiguous()
    return F.conv2d(img, w2.to(device=img.device, dtype=img.dtype), padding=pad, groups=c)


def ssim_map(img1, img2, window_size=11, separable=False):
    conv = lambda t: _convolve(t, window_size, separable)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def ssim(img1, img2, window_size=11, size_average=True, separable=False):
    m = ssim_map(img1, img2, window_size, separable)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def img2mse(x, y, mask=None):
    """x, y [..., C], mask [...]"""
    if mask is None:
        return torch.mean((x - y) * (x - y))
    return torch.sum((x - y) * (x - y) * mask.unsqueeze(-1)) / (torch.sum(mask) * x.shape[-1] + TINY_NUMBER)


def mse2psnr(mse):
    return -10.0 * torch.log10(mse + TINY_NUMBER)


def image_loss_reference(pred, target, mask=None, window_size=11, size_average=True, separable=False):
    """(mse, ssim): shape [] with size_average, otherwise [B]"""
    x, y = pred.permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)
    if size_average:
        mse = img2mse(x, y, mask)
    else:
        mse = torch.stack([img2mse(x[b], y[b], None if mask is None else mask[b]) for b in range(pred.shape[0])])
    return mse, ssim(pred, target, window_size, size_average, separable)


def make_image_case(b, c, h, w, noise, seed, masked):
    """float64 tensors whose values are float32 numbers: target uniform in [0, 1], pred = clamp(target + noise * randn, 0, 1), the
    mask in {0, 0.5, 1} per pixel (or None), and one fixed upstream gradient per image for each result (with size_average the
    first is used)."""
    gen = torch.Generator().manual_seed(seed)
    f32 = lambda t: t.float().double()
    target = f32(torch.rand(b, c, h, w, generator=gen, dtype=torch.float64))
    pred = f32((target + noise * torch.randn(b, c, h, w, generator=gen, dtype=torch.float64)).clamp(0, 1))
    mask = 0.5 * torch.randint(0, 3, (b, h, w), generator=gen).double() if masked else None
    g_mse = f32(0.5 + torch.rand(b, generator=gen, dtype=torch.float64))
    g_ssim = f32(-0.5 - torch.rand(b, generator=gen, dtype=torch.float64))
    return dict(pred=pred, target=target, mask=mask, g_mse=g_mse, g_ssim=g_ssim)


def run_image_loss(fn, case, dtype, device, window_size=11, size_average=True, use=("mse", "ssim"), target_grad=True, **more):
    """`fn(pred, target, mask, window_size=, size_average=)` -> (mse, ssim) on the case in `dtype` on `device`; the loss is
    sum(g_mse * mse) + sum(g_ssim * ssim) over the results in `use`.  Returns mse, ssim, d_pred (and d_target), detached."""
    to = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)      # (a new leaf: the case stays as it is)
    pred, target = to(case["pred"]).requires_grad_(True), to(case["target"]).requires_grad_(target_grad)
    mse, ssim_ = fn(pred, target, to(case["mask"]), window_size=window_size, size_average=size_average, **more)
    n = mse.numel()
    loss = 0
    if "mse" in use:
        loss = loss + (mse.reshape(-1) * to(case["g_mse"])[:n]).sum()
    if "ssim" in use:
        loss = loss + (ssim_.reshape(-1) * to(case["g_ssim"])[:n]).sum()
    grads = torch.autograd.grad(loss, [pred, target] if target_grad else [pred])
    out = dict(mse=mse.detach(), ssim=ssim_.detach(), d_pred=grads[0])
    if target_grad:
        out["d_target"] = grads[1]
    return out
