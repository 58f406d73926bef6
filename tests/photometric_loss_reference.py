"""A restatement in torch of what `fused_photometric_loss` replaces — GGRt's `MultiViewPhotometricDecayLoss.forward`
(ggrt/loss/photometric_loss.py) with the geometry it calls (`Camera.reconstruct` / `.project`, `inv2depth`, `calc_smoothness`,
`Pose.from_vec`) — written from their semantics for batch 1, the 'min' reduce, zeros padding and SSIM on, in any dtype on any
device, and pinned to the reference's own modules by tests/test_photometric_loss_reference.py (fixtures: tests/golden/).

With `decisions=(choice, unclamped)` the per-pixel minimum and the clamp are not decided here: the winner of pixel q of iteration i
is candidate `choice[i, q]`, and its value is p where `unclamped[i, q]`, the threshold (a constant) elsewhere.  That is how the GPU
test compares gradients without the flips of near-ties."""
import math

import torch
import torch.nn.functional as F

DEFAULTS = dict(ssim_loss_weight=0.85, smooth_loss_weight=0.01, C1=1e-4, C2=9e-4, clip_loss=0.5, automask_loss=True, gamma=0.85)


def euler_to_R(angle):
    """[B,3] Euler angles -> [B,3,3], R = Rx Ry Rz."""
    x, y, z = angle[:, 0], angle[:, 1], angle[:, 2]
    o, l = torch.zeros_like(x), torch.ones_like(x)
    rz = torch.stack([z.cos(), -z.sin(), o, z.sin(), z.cos(), o, o, o, l], 1).view(-1, 3, 3)
    ry = torch.stack([y.cos(), o, y.sin(), o, l, o, -y.sin(), o, y.cos()], 1).view(-1, 3, 3)
    rx = torch.stack([l, o, o, o, x.cos(), -x.sin(), o, x.sin(), x.cos()], 1).view(-1, 3, 3)
    return rx @ ry @ rz


def sample_coordinates(inv_depth, K, ref_K, pose6):
    """The pixel coordinates (u, v) [H,W] each at which the reference view is sampled: lift with Kinv and 1/inv_depth (inv2depth),
    move by the pose, project with ref_K, Z clamped at 1e-5."""
    H, W = inv_depth.shape[-2:]
    dt, dev = inv_depth.dtype, inv_depth.device
    kinv = K.reshape(3, 3).clone()
    kinv[0, 0] = 1.0 / K.reshape(3, 3)[0, 0]
    kinv[1, 1] = 1.0 / K.reshape(3, 3)[1, 1]
    kinv[0, 2] = -1.0 * K.reshape(3, 3)[0, 2] / K.reshape(3, 3)[0, 0]
    kinv[1, 2] = -1.0 * K.reshape(3, 3)[1, 2] / K.reshape(3, 3)[1, 1]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    grid = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)
    d = inv_depth.reshape(1, -1)
    depth = torch.where(d <= 0, torch.zeros_like(d), 1.0 / d.clamp(min=1e-6))
    X = (kinv @ grid) * depth
    R = euler_to_R(pose6[None, 3:])[0]
    Y = R @ X + pose6[:3, None]
    P = ref_K.reshape(3, 3) @ Y
    Z = P[2].clamp(min=1e-5)
    return (P[0] / Z).reshape(H, W), (P[1] / Z).reshape(H, W)


def warp(ref_img, u, v):
    """grid_sample(bilinear, zeros, align_corners=True) of ref_img [3,H,W] at the normalised (u, v), as the reference normalises."""
    H, W = u.shape
    grid = torch.stack([2 * u / (W - 1) - 1.0, 2 * v / (H - 1) - 1.0], -1)[None]
    return F.grid_sample(ref_img[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]


def candidate(x, image, w, C1, C2):
    """p [H,W] of one candidate image x [3,H,W] against image [3,H,W]: w * mean_c SSIM loss + (1 - w) * mean_c L1."""
    xp, yp = F.pad(x[None], (1, 1, 1, 1), mode="reflect"), F.pad(image[None], (1, 1, 1, 1), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 3, stride=1)
    mu_x, mu_y = pool(xp), pool(yp)
    sig_x, sig_y, sig_xy = pool(xp * xp) - mu_x * mu_x, pool(yp * yp) - mu_y * mu_y, pool(xp * yp) - mu_x * mu_y
    ssim = ((2 * mu_x * mu_y + C1) * (2 * sig_xy + C2)) / ((mu_x * mu_x + mu_y * mu_y + C1) * (sig_x + sig_y + C2))
    ssim_loss = torch.clamp((1.0 - ssim) / 2.0, 0.0, 1.0)
    return (w * ssim_loss.mean(1) + (1 - w) * (x[None] - image[None]).abs().mean(1))[0]


def photometric_loss_reference(image, ref_imgs, inv_depths, K, ref_Ks, poses, *, ssim_loss_weight=0.85, smooth_loss_weight=0.01,
                               C1=1e-4, C2=9e-4, clip_loss=0.5, automask_loss=True, gamma=0.85, decisions=None):
    """image [1,3,H,W], ref_imgs [V,3,H,W], inv_depths [n,1,H,W], K [1,3,3], ref_Ks [V,3,3], poses [V,n,6] -> dict."""
    img = image.reshape(3, *image.shape[-2:])
    n, V = inv_depths.shape[0], ref_imgs.shape[0]
    H, W = img.shape[-2:]
    unwarped = [candidate(ref_imgs[j], img, ssim_loss_weight, C1, C2) for j in range(V)] if automask_loss else None
    planes, coords = [], []
    for i in range(n):
        row, uv = [], []
        for j in range(V):
            u, v = sample_coordinates(inv_depths[i, 0], K, ref_Ks[j], poses[j, i])
            uv.append(torch.stack([u, v]))
            row.append(candidate(warp(ref_imgs[j], u, v), img, ssim_loss_weight, C1, C2))
            if automask_loss:
                row.append(unwarped[j])
        planes.append(torch.stack(row))
        coords.append(torch.stack(uv))
    P = torch.stack(planes)                                   # [n,C,H,W]
    coords = torch.stack(coords).detach()                     # [n,V,2,H,W]
    thr = (P.mean((2, 3)) + clip_loss * P.std((2, 3))).detach()          # [n,C]: a constant of the backward (the reference's float())
    thr_full = thr[:, :, None, None].expand_as(P)
    if decisions is None:
        clamped = torch.minimum(P, thr_full) if clip_loss > 0 else P
        best = clamped.min(1, keepdim=True)[0]
        choice = (clamped == best).to(torch.uint8).argmax(1)          # ties: the lowest index
        unclamped = (P.gather(1, choice[:, None])[:, 0] <= thr_full.gather(1, choice[:, None])[:, 0]) if clip_loss > 0 else torch.ones_like(choice, dtype=torch.bool)
    else:
        choice, unclamped = decisions[0].to(device=P.device, dtype=torch.long), decisions[1].to(device=P.device, dtype=torch.bool)
        clamped = None
    value = torch.where(unclamped, P.gather(1, choice[:, None])[:, 0], thr_full.gather(1, choice[:, None])[:, 0])
    weights = torch.tensor([gamma ** (n - i - 1) for i in range(n)], dtype=P.dtype, device=P.device)
    photometric = (weights * value.mean((1, 2))).sum()
    smoothness = torch.zeros((), dtype=P.dtype, device=P.device)
    if smooth_loss_weight > 0:
        for i in range(n):
            d = inv_depths[i:i + 1]
            dn = d / d.mean(2, True).mean(3, True).clamp(min=1e-6)
            gx, gy = dn[..., :, :-1] - dn[..., :, 1:], dn[..., :-1, :] - dn[..., 1:, :]
            im = img[None]
            wx = torch.exp(-(im[..., :, :-1] - im[..., :, 1:]).abs().mean(1, keepdim=True))
            wy = torch.exp(-(im[..., :-1, :] - im[..., 1:, :]).abs().mean(1, keepdim=True))
            smoothness = smoothness + ((gx * wx).abs().mean() + (gy * wy).abs().mean()) / 2 ** i
        smoothness = smooth_loss_weight * (smoothness / n)
    loss = (photometric + smoothness).unsqueeze(0) if smooth_loss_weight > 0 else photometric.unsqueeze(0)
    # the reference's metric is `photometric.detach()`, which shares its memory with the tensor that `loss += smoothness` then changes in
    # place: with the smoothness term on, the 'photometric_loss' metric IS the whole loss
    return dict(loss=loss, photometric_loss=loss[0].detach(), smoothness_loss=smoothness.detach(), thresholds=thr, choice=choice.to(torch.uint8),
                unclamped=unclamped, planes=P.detach(), clamped=None if clamped is None else clamped.detach(), coords=coords)


def _texture(xs, ys, g, scale=1.0):
    """A smooth field with strong local variance, evaluated at continuous pixel coordinates: values in about [0.1, 0.9] x 3."""
    out = []
    for _ in range(3):
        f = torch.zeros_like(xs)
        for k in range(4):
            fx, fy = (torch.rand(2, generator=g, dtype=torch.float64) * 1.0 + 0.35) / scale
            ph = torch.rand(1, generator=g, dtype=torch.float64) * 6.28
            f = f + torch.sin(fx * xs + fy * ys * (1 if k % 2 else -1) + ph) / 4
        out.append(0.5 + 0.4 * f)
    return torch.stack(out)


def make_photometric_case(V, n, H, W, seed, identity=False, far_view=None, shift=1.6):
    """Seeded float64 CPU inputs.  The reference views are the target's texture moved by about `shift` pixels (plus noise), the
    inverse depths a smooth field inside [0.35, 0.65] that changes a little with the iteration, the poses the translations that undo
    most of the move plus small angles, except in a corner region that every view shows unmoved: warped and unwarped candidates both win somewhere, some samples leave the frame, and the
    clip acts.  `identity`: exact zero poses, constant inverse depth 0.5 and power-of-two intrinsics, for which the warped image IS
    the reference image bit for bit.  `far_view`: that view's poses throw every sample out of frame."""
    g = torch.Generator().manual_seed(seed)
    f = 16.0 if identity else 0.8 * max(W, 8)
    cx, cy = (float((W - 1) // 2), float((H - 1) // 2)) if identity else ((W - 1) / 2.0 + 0.13, (H - 1) / 2.0 - 0.21)
    K = torch.tensor([[[f, 0, cx], [0, f, cy], [0, 0, 1]]], dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    tstate = g.get_state()
    tex = lambda sx, sy: (g.set_state(tstate), _texture(xs + sx, ys + sy, g))[1]
    noise = lambda: 0.04 * (torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed * 7919 + noise.k), dtype=torch.float64) - 0.5)
    noise.k = 0
    image = (tex(0.0, 0.0) + noise()).clamp(0, 1)
    outlier = ((xs * 7 + ys * 13) % 23 == 5)               # isolated pixels that no view explains: every candidate is large there, the clip acts
    image = torch.where(outlier, 1.0 - image, image)[None]
    static = (xs < 0.3 * W) if W >= H else (ys < 0.3 * H)          # a part of the scene that moves with the camera: there the unwarped image wins
    refs, ref_Ks, poses = [], [], []
    base = 0.5 + 0.15 * torch.sin(xs / max(W, 4) * 3.1 + 0.4) * torch.cos(ys / max(H, 4) * 2.3)
    for j in range(V):
        noise.k = j + 1
        ang = 2.39996 * j + 0.7
        sx, sy = shift * math.cos(ang) * (1 + 0.3 * j) * min(1.0, W / 16.0), 0.45 * shift * math.sin(ang) * min(1.0, H / 16.0)
        if identity:
            sx = sy = 0.0
        moved = tex(sx, sy)
        refs.append((torch.where(static, tex(0.0, 0.0), moved) + noise()).clamp(0, 1))
        kj = K[0].clone()
        if not identity:
            kj[0, 0] *= 1 + 0.01 * (j + 1)
            kj[1, 1] *= 1 - 0.008 * (j + 1)
            kj[0, 2] += 0.3 * j
        ref_Ks.append(kj)
        per_iter = []
        for i in range(n):
            if identity:
                per_iter.append(torch.zeros(6, dtype=torch.float64))
                continue
            conv = 1.0 - 0.5 * (n - 1 - i) / max(n, 1)       # the iterations approach the move
            # a point at inverse depth 0.5 moves by f * t * 0.5 pixels; target pixel q shows up in the reference view at q - (sx, sy)
            t = torch.tensor([-sx * conv / (0.5 * f), -sy * conv / (0.5 * f), 0.02 * math.sin(i + j)], dtype=torch.float64)
            r = 0.004 * torch.tensor([math.sin(1.3 * i + j), math.cos(0.7 * i - j), math.sin(0.5 * i + 2 * j)], dtype=torch.float64)
            if far_view is not None and j == far_view:
                t = t + torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64)
            per_iter.append(torch.cat([t, r]))
        poses.append(torch.stack(per_iter))
    inv = []
    for i in range(n):
        if identity:
            inv.append(torch.full((1, H, W), 0.5, dtype=torch.float64))
        else:
            inv.append((base + 0.03 * torch.sin(xs * 0.9 + i) * torch.sin(ys * 1.1 - 0.5 * i) + 0.01 * i / max(n, 1))[None])
    return dict(image=image, ref_imgs=torch.stack(refs), inv_depths=torch.stack(inv), K=K, ref_Ks=torch.stack(ref_Ks), poses=torch.stack(poses))


def run_photometric_loss(route, case, dtype, device, decisions=None, grad_out=1.0, need=("inv_depths", "poses"), **opts):
    """`route` is "torch" (the restatement) or a callable with `fused_photometric_loss`'s signature.  Returns a dict of detached
    results: loss, photometric_loss, smoothness_loss, thresholds, choice, g_inv_depths [n,1,H,W], g_poses [V,n,6] (None where not in
    `need`), and for the restatement also unclamped, planes, clamped and coords."""
    t = {k: v.detach().to(device=device, dtype=dtype).clone() for k, v in case.items()}
    t["inv_depths"].requires_grad_("inv_depths" in need)
    t["poses"].requires_grad_("poses" in need)
    args = (t["image"], t["ref_imgs"], t["inv_depths"], t["K"], t["ref_Ks"], t["poses"])
    if route == "torch":
        out = photometric_loss_reference(*args, decisions=decisions, **opts)
    else:
        got = route(*args, return_choice=True, **opts)
        out = dict(loss=got.loss, photometric_loss=got.photometric_loss, smoothness_loss=got.smoothness_loss, thresholds=got.thresholds, choice=got.choice)
    (out["loss"] * grad_out).sum().backward()
    res = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    res["g_inv_depths"] = t["inv_depths"].grad
    res["g_poses"] = t["poses"].grad
    return res


def decided_pixels(ref, delta, clip_loss=0.5):
    """[n,H,W] bool from the float64 restatement's result: the best and second-best clamped candidates differ by more than delta,
    every candidate is more than delta from its threshold, and every view's sample coordinate is more than 2e-4 px from an integer
    line (the image border is one) unless it is out of frame by more than that anyway."""
    clamped, P, thr = ref["clamped"], ref["planes"], ref["thresholds"]
    ok = torch.ones(P.shape[0], *P.shape[2:], dtype=torch.bool)
    if P.shape[1] > 1:
        two = clamped.topk(2, dim=1, largest=False)[0]
        ok &= (two[:, 1] - two[:, 0]) > delta
    if clip_loss > 0:
        ok &= ((P - thr[:, :, None, None]).abs() > delta).all(1)
    H, W = P.shape[-2:]
    for axis, size in ((0, W), (1, H)):
        c = ref["coords"][:, :, axis]
        near = ((c - c.round()).abs() <= 2e-4) & (c >= -1.001) & (c <= size + 0.001)
        ok &= ~near.any(1)
    return ok
