"""A torch restatement of GGRt's convex depth upsampling (ggrt/depth_pose_network.py: `DepthPoseNet.upsample_depth`, optionally
followed by `disp_to_depth(...)[0]` of ggrt/geometry/depth.py), written out step by step in the dtype of its inputs, and a seeded
case maker.  tests/golden/upsample_depth_*.npz (made from the reference's own method by tests/golden/make_upsample_depth_golden.py)
pin it; the GPU tests hold `fused_upsample_depth` against it in float64.

    p    = softmax over the 9 taps k of mask[n, k r r + i r + j, y, x]        (the maximum subtracted first)
    up[n, y r + i, x r + j] = sum_k p_k depth[n, y + ky - 1, x + kx - 1]      (zero outside the map; k = ky 3 + kx)
    out  = bilinear resize of up, align_corners: source = destination * (in - 1) / (out - 1), 0 for one destination index;
           weights (1 - l, l); the neighbour clamped at the last row and column
    out  = 1/max_depth + (1/min_depth - 1/max_depth) out                      with disp_range"""
import torch
import torch.nn.functional as F

INPUTS = ("depth", "mask")


def convex_upsample(depth, mask, ratio):
    """depth [N,1,h,w], mask [N,9 r r,h,w] -> up [N,1,r h,r w]"""
    N, _, h, w = depth.shape
    r = int(ratio)
    m = mask.reshape(N, 9, r, r, h, w)
    e = torch.exp(m - m.amax(dim=1, keepdim=True))
    p = e / e.sum(dim=1, keepdim=True)
    padded = F.pad(depth[:, 0], (1, 1, 1, 1))
    taps = torch.stack([padded[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)        # [N,9,h,w]
    up = (p * taps[:, :, None, None]).sum(1)                                                                  # [N,r(i),r(j),h,w]
    return up.permute(0, 3, 1, 4, 2).reshape(N, 1, r * h, r * w)


def _axis(n_in, n_out, dtype, device):
    # the scale is a true division in `dtype` on the host, as torch (and the kernel's argument set-up) forms it: on the device a tensor
    # divided by a number is multiplied by the reciprocal, and 55 * (1 / 55) is not 1 in float32
    scale = torch.tensor(float(n_in - 1), dtype=dtype) / torch.tensor(float(n_out - 1), dtype=dtype) if n_out > 1 else torch.zeros((), dtype=dtype)
    src = scale.to(device) * torch.arange(n_out, dtype=dtype, device=device)
    # torch's CPU guard: the index is floorf of the coordinate whatever the dtype, the weight clamped to [0, 1].  Nothing in float32;
    # in float64 a coordinate one ulp below an integer (49 * (55 / 49)) takes that integer with weight 0, not its lower neighbour
    i0 = src.float().floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = (src - i0.to(dtype)).clamp(0, 1)
    return i0, i1, 1 - l1, l1


def bilinear_resize(up, size):
    """F.interpolate(up, size, mode="bilinear", align_corners=True), with torch's own source-index arithmetic in up's dtype"""
    H, W = up.shape[-2:]
    Ho, Wo = size
    y0, y1, ly0, ly1 = _axis(H, Ho, up.dtype, up.device)
    x0, x1, lx0, lx1 = _axis(W, Wo, up.dtype, up.device)
    top, bot = up[..., y0, :], up[..., y1, :]
    row = lambda t: lx0 * t[..., x0] + lx1 * t[..., x1]
    return ly0[:, None] * row(top) + ly1[:, None] * row(bot)


def upsample_depth_reference(depth, mask, ratio=8, image_size=None, disp_range=None):
    if depth.dim() == 3:
        depth = depth.unsqueeze(1)
    N, _, h, w = depth.shape
    up = convex_upsample(depth, mask, ratio)
    out = bilinear_resize(up, image_size if image_size is not None else (ratio * h, ratio * w))
    if disp_range is not None:
        lo, hi = 1.0 / disp_range[1], 1.0 / disp_range[0]
        out = lo + (hi - lo) * out
    return out


def make_upsample_case(N, h, w, r, size, seed):
    """Seeded float64 CPU inputs: a raw sigmoid disparity in (0.05, 0.95), logits of a few units, and the upstream gradient `g`
    [N,1,Ho,Wo] the tests multiply the output with.  `size` None is the identity size."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = size if size is not None else (r * h, r * w)
    return dict(depth=0.05 + 0.9 * torch.rand(N, 1, h, w, generator=g, dtype=torch.float64),
                mask=3.0 * torch.randn(N, 9 * r * r, h, w, generator=g, dtype=torch.float64),
                g=torch.rand(N, 1, Ho, Wo, generator=g, dtype=torch.float64) + 0.5)


def run_upsample_depth(route, case, dtype, device, need=INPUTS, **opts):
    """`route` is "torch" (the restatement) or a callable with `fused_upsample_depth`'s signature.  The loss is sum(out * g).
    Returns a dict of detached results: out, g_depth, g_mask (None where not in `need`)."""
    t = {k: v.detach().to(device=device, dtype=dtype).clone() for k, v in case.items()}
    for k in INPUTS:
        t[k].requires_grad_(k in need)
    fn = upsample_depth_reference if route == "torch" else route
    out = fn(t["depth"], t["mask"], **opts)
    if need:
        (out * t["g"]).sum().backward()
    res = dict(out=out.detach())
    for k in INPUTS:
        res["g_" + k] = t[k].grad
    return res
