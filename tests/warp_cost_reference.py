"""A restatement in torch of what `fused_warp_cost` replaces — GGRt's `DepthPoseNet.get_cost_each` / `depth_cost_calc`
(ggrt/depth_pose_network.py) with the geometry they call (`Camera.scaled` / `.reconstruct` / `.project`, `inv2depth`, `disp_to_depth`,
`Pose.from_vec`) — written from their semantics for batch 1, in any dtype on any device, and pinned to the reference's own methods by
tests/test_warp_cost_reference.py (fixtures: tests/golden/warp_cost_*.npz).

With `decisions=cells` ([V,h,w,3] integers: floor u, floor v, the P.z-clamped flag) the bilinear cell and the clamp are not decided
here: the taps are those of the given cell, with the weights u - ix and v - iy, and Z is the constant 1e-5 where the flag is set.
Bilinear interpolation is continuous across a cell border and max(P.z, 1e-5) across the clamp, so the value changes only by
rounding; the one-sided derivative becomes that of the given cell.  That is how the GPU tests compare gradients on pixels whose
coordinate sits within float32 rounding of an integer."""
import math

import torch


def euler_to_R(angle):
    """[B,3] Euler angles -> [B,3,3], R = Rx Ry Rz."""
    x, y, z = angle[:, 0], angle[:, 1], angle[:, 2]
    o, l = torch.zeros_like(x), torch.ones_like(x)
    rz = torch.stack([z.cos(), -z.sin(), o, z.sin(), z.cos(), o, o, o, l], 1).view(-1, 3, 3)
    ry = torch.stack([y.cos(), o, y.sin(), o, l, o, -y.sin(), o, y.cos()], 1).view(-1, 3, 3)
    rx = torch.stack([l, o, o, o, x.cos(), -x.sin(), o, x.sin(), x.cos()], 1).view(-1, 3, 3)
    return rx @ ry @ rz


def scaled_K(K, s):
    """scale_intrinsics on a clone; Camera.scaled returns the camera itself for a factor of exactly 1."""
    K = K.reshape(3, 3).clone()
    if s == 1.0:
        return K
    K[0, 0] = K[0, 0] * s
    K[1, 1] = K[1, 1] * s
    K[0, 2] = (K[0, 2] + 0.5) * s - 0.5
    K[1, 2] = (K[1, 2] + 0.5) * s - 0.5
    return K


def projected(inv_depth, K, ref_K, pose6, scale_factor, disp_range=None):
    """P [3,h,w] = Kref' (R X + t) of every pixel: disp_to_depth (when folded), inv2depth, lift with Kinv of the scaled K, move, project."""
    h, w = inv_depth.shape[-2:]
    dt, dev = inv_depth.dtype, inv_depth.device
    Ks = scaled_K(K, scale_factor)
    kinv = Ks.clone()
    kinv[0, 0] = 1.0 / Ks[0, 0]
    kinv[1, 1] = 1.0 / Ks[1, 1]
    kinv[0, 2] = -1.0 * Ks[0, 2] / Ks[0, 0]
    kinv[1, 2] = -1.0 * Ks[1, 2] / Ks[1, 1]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt, device=dev), torch.arange(w, dtype=dt, device=dev), indexing="ij")
    grid = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)
    d = inv_depth.reshape(1, -1)
    if disp_range is not None:
        lo, hi = 1.0 / disp_range[1], 1.0 / disp_range[0]
        d = lo + (hi - lo) * d
    depth = torch.where(d <= 0, torch.zeros_like(d), 1.0 / d.clamp(min=1e-6))
    X = (kinv @ grid) * depth
    R = euler_to_R(pose6[None, 3:])[0]
    Y = R @ X + pose6[:3, None]
    return (scaled_K(ref_K, scale_factor) @ Y).reshape(3, h, w)


def bilinear(ref, u, v, cell=None):
    """grid_sample(bilinear, zeros, align_corners=True) of ref [C,h,w] at the pixel coordinates (u, v) [h,w] each, tap by tap; with
    `cell` = (ix, iy) the taps are those of that cell."""
    C, h, w = ref.shape
    if cell is None:
        uc, vc = u.clamp(-2.0, w + 1.0), v.clamp(-2.0, h + 1.0)          # (beyond these no tap is reached either way)
        uc, vc = torch.where(torch.isnan(u), torch.full_like(u, -2.0), uc), torch.where(torch.isnan(v), torch.full_like(v, -2.0), vc)
        ix, iy = uc.detach().floor().long(), vc.detach().floor().long()
    else:
        uc, vc = u, v
        ix, iy = cell[0].long(), cell[1].long()
    wx1, wy1 = uc - ix.to(u.dtype), vc - iy.to(u.dtype)
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    flat = ref.reshape(C, h * w)
    out = torch.zeros(C, h, w, dtype=ref.dtype, device=ref.device)
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            x, y = ix + dx, iy + dy
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            idx = (y.clamp(0, h - 1) * w + x.clamp(0, w - 1)).reshape(-1)
            val = flat[:, idx].reshape(C, h, w)
            out = out + torch.where(ok, wx * wy, torch.zeros_like(wx))[None] * torch.where(ok[None], val, torch.zeros_like(val))
    return out


def warp_cost_reference(fmap, fmaps_ref, inv_depth, K, ref_Ks, poses, *, scale_factor=1.0 / 8, reduce="mean", disp_range=None, decisions=None):
    """fmap [1,C,h,w], fmaps_ref [V,C,h,w], inv_depth [1,1,h,w], K [1,3,3], ref_Ks [V,3,3], poses [V,6] -> dict: cost ([1,C,h,w] for
    "mean", [V,C,h,w] for "none"), coords [V,2,h,w], pz [V,h,w], cells [V,h,w,3] (this run's own, or the injected ones)."""
    V = fmaps_ref.shape[0]
    f = fmap.reshape(fmap.shape[-3:])
    costs, coords, pz, cells = [], [], [], []
    for j in range(V):
        P = projected(inv_depth, K, ref_Ks[j], poses[j], scale_factor, disp_range)
        if decisions is None:
            clamped = ~(P[2].detach() >= 1e-5)
            cell = None
        else:
            dj = decisions[j].to(P.device)
            clamped = dj[..., 2] != 0
            cell = (dj[..., 0], dj[..., 1])
        Z = torch.where(clamped, torch.full_like(P[2], 1e-5), P[2])
        u, v = P[0] / Z, P[1] / Z
        fw = bilinear(fmaps_ref[j], u, v, cell)
        costs.append((f - fw) ** 2)
        coords.append(torch.stack([u, v]).detach())
        pz.append(P[2].detach())
        if decisions is None:
            h, w = u.shape
            inside = (u.detach() > -1) & (u.detach() < w) & (v.detach() > -1) & (v.detach() < h)
            minus2 = torch.full(u.shape, -2, dtype=torch.long, device=u.device)
            cells.append(torch.stack([torch.where(inside, u.detach().clamp(-2, w + 1).floor().long(), minus2),
                                      torch.where(inside, v.detach().clamp(-2, h + 1).floor().long(), minus2), clamped.long()], -1))
        else:
            cells.append(decisions[j].long())
    costs = torch.stack(costs)
    cost = costs.mean(0, keepdim=True) if reduce == "mean" else costs
    return dict(cost=cost, coords=torch.stack(coords), pz=torch.stack(pz), cells=torch.stack(cells).to(torch.int32))


def _texture(xs, ys, g, channels, amp=0.4):
    """Smooth fields with strong local variance, evaluated at continuous pixel coordinates: one per channel, values about 0.5 +- amp."""
    out = []
    for _ in range(channels):
        f = torch.zeros_like(xs)
        for k in range(3):
            fx, fy = torch.rand(2, generator=g, dtype=torch.float64) * 0.9 + 0.3
            ph = torch.rand(1, generator=g, dtype=torch.float64) * 6.28
            f = f + torch.sin(fx * xs + fy * ys * (1 if k % 2 else -1) + ph) / 3
        out.append(0.5 + amp * f)
    return torch.stack(out)


DEPTH_COLUMN_VALUES = (1e-7, 1e-6, 1.0000001e-6, 1e3, 0.0, -1.0)          # the rows of `depth_column` cycle through these inverse depths


def depth_class(d):
    """0 where the depth is the constant 0 (d <= 0), 1 where it is the clamp's constant (0 < d < 1e-6), 2 where it is 1 / d."""
    return (d > 0).long() + (d >= 1e-6).long()


def folded32(x, disp_range):
    """disp_to_depth's affine map as float32 evaluates it (the restatement's own expression on a float32 tensor)."""
    lo, hi = 1.0 / disp_range[1], 1.0 / disp_range[0]
    return lo + (hi - lo) * x.to(torch.float32)


def _raw_disparity(value, disp_range):
    """The float32 number x for which d = lo + (hi - lo) x comes nearest to `value` among those (within 4096 float32 steps of the
    exact raw disparity) for which float32 and float64 evaluate d alike: on `value`'s side of 0 and of the 1e-6 clamp in both, and,
    where the depth is 1 / d, equal to 2^-22 of d.  Near lo the float32 fold moves in steps of about 2^-30, a thousandth of 1e-6:
    for any other x the side of the gate, and the depth of 1e6 behind it, would be decided by rounding, differently in the two
    precisions.  Needs a `disp_range` whose 1 / max and 1 / min - 1 / max are float32 numbers, such as (1, 128)."""
    lo, hi = 1.0 / disp_range[1], 1.0 / disp_range[0]
    want = int(depth_class(torch.tensor(value, dtype=torch.float64)))
    x = torch.tensor([(value - lo) / (hi - lo)], dtype=torch.float64).to(torch.float32)
    cands = (x.view(torch.int32) + torch.arange(-4096, 4097, dtype=torch.int32)).view(torch.float32)
    d64, d32 = lo + (hi - lo) * cands.double(), folded32(cands, disp_range)
    ok = (depth_class(d64) == want) & (depth_class(d32) == want)          # (float32 against the float32 1e-6, as the kernel compares)
    if want == 2:
        ok &= (d32.double() - d64).abs() <= 2.0 ** -22 * d64.abs()
    assert bool(ok.any()), (value, disp_range)
    return float(cands[ok][(d64[ok] - value).abs().argmin()])


def make_warp_case(V, C, h, w, seed, scale_factor=1.0 / 8, identity=False, far_view=None, behind_view=None, nonpositive_block=False, disp_range=None,
                   same_K=False, angles=None, straddle_view=None, depth_column=None, collapse=False):
    """Seeded float64 CPU inputs with smooth feature maps and moderate poses (shifts of one to two pixels, angles of a few
    milliradians), FULL-resolution intrinsics that differ per view, an inverse depth inside [0.35, 0.65] (with `disp_range` the raw
    disparity that maps there), and the upstream gradients `g_mean` [1,C,h,w] and `g_none` [V,C,h,w] the tests multiply the cost
    with.  `identity`: zero poses, equal power-of-two intrinsics and inverse depth 0.5, for which u = x and v = y exactly.
    `far_view`: that view's samples all leave the frame.  `behind_view`: that view's points lie behind its camera (P.z < 0).
    `nonpositive_block`: a corner block of the inverse depth is 0 and negative.
    `angles` (V triples, radians): view j gets those Euler angles and the translation Xc - R Xc + t, with Xc the centre pixel lifted
    with the scaled K to depth 2 and t the translation drawn otherwise: the centre stays put and the frame turns about it.
    `straddle_view`: that view's t_z is minus a depth inside the map's range, so that P.z changes sign across the map, and its focal
    length is STRADDLE_FOCAL of the others' (see there).
    `depth_column`: that column of the inverse depth cycles through DEPTH_COLUMN_VALUES down its rows (with `disp_range`: through
    the float32 raw disparities that `_raw_disparity` finds for them), and every t_z grows by 1 so that a point at depth 0 or 1e-3
    still projects into the frame: what keeps its dL/dinv_depth at zero is the gate, not a sample that reaches nothing.
    `collapse`: fmap = 2 (above every reference value, so fmap - warped > 0), inverse depth 1e4 (depth 1e-4, X about 0), t_z = 1 and
    t_x, t_y such that Kr t / t_z = (w // 2 + 0.3, h // 2 + 0.6): every pixel samples that one cell."""
    g = torch.Generator().manual_seed(seed)
    s = float(scale_factor)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    if identity:
        f_s, cx_s, cy_s = 16.0, float((w - 1) // 2), float((h - 1) // 2)
    else:
        f_s, cx_s, cy_s = 0.8 * max(w, 8), (w - 1) / 2.0 + 0.13, (h - 1) / 2.0 - 0.21
    full = lambda f, cx, cy: torch.tensor([[f / s, 0, (cx + 0.5) / s - 0.5], [0, f / s, (cy + 0.5) / s - 0.5], [0, 0, 1]], dtype=torch.float64)
    K = full(f_s, cx_s, cy_s)[None]
    tstate = g.get_state()
    tex = lambda sx, sy: (g.set_state(tstate), _texture(xs + sx, ys + sy, g, C))[1]
    fmap = tex(0.0, 0.0)[None]
    g2 = torch.Generator().manual_seed(seed * 7919 + 1)
    refs, ref_Ks, poses = [], [], []
    for j in range(V):
        ang = 2.39996 * j + 0.7
        sx, sy = 1.6 * math.cos(ang) * min(1.0, w / 16.0), 0.9 * math.sin(ang) * min(1.0, h / 16.0)
        if identity:
            refs.append(_texture(xs, ys, g2, C))
            ref_Ks.append(K[0].clone())
            poses.append(torch.zeros(6, dtype=torch.float64))
            continue
        refs.append(tex(sx, sy) + 0.15 * (_texture(xs, ys, g2, C) - 0.5))
        ref_Ks.append(K[0].clone() if same_K else full(f_s * (1 + 0.01 * (j + 1)), cx_s + 0.3 * j, cy_s - 0.2 * j))
        ref_Ks[-1][1, 1] *= 1.0 if same_K else 1 - 0.008 * (j + 1)
        t = torch.tensor([-sx * 0.7 / (0.5 * f_s), -sy * 0.7 / (0.5 * f_s), 0.02 * math.sin(1.0 + j)], dtype=torch.float64)
        r = 0.004 * torch.tensor([math.sin(1.3 + j), math.cos(0.7 - j), math.sin(0.5 + 2 * j)], dtype=torch.float64)
        if far_view is not None and j == far_view:
            t = t + torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64)
        if behind_view is not None and j == behind_view:
            t = t + torch.tensor([0.0, 0.0, -6.0], dtype=torch.float64)
        if angles is not None:
            r = torch.tensor(angles[j], dtype=torch.float64)
            Xc = 2.0 * torch.tensor([((w - 1) / 2.0 - cx_s) / f_s, ((h - 1) / 2.0 - cy_s) / f_s, 1.0], dtype=torch.float64)
            t = Xc - euler_to_R(r[None])[0] @ Xc + t
        if straddle_view is not None and j == straddle_view:
            t[2] = -STRADDLE_DEPTH
            ref_Ks[-1][0, 0] *= STRADDLE_FOCAL
            ref_Ks[-1][1, 1] *= STRADDLE_FOCAL
        if depth_column is not None:
            t[2] = t[2] + 1.0
        if collapse:
            Kr = scaled_K(ref_Ks[-1], s)
            t = torch.stack([(w // 2 + 0.3 - Kr[0, 2]) / Kr[0, 0], (h // 2 + 0.6 - Kr[1, 2]) / Kr[1, 1], torch.tensor(1.0, dtype=torch.float64)])
        poses.append(torch.cat([t, r]))
    d = torch.full((h, w), 0.5, dtype=torch.float64) if identity else 0.5 + 0.15 * torch.sin(xs / max(w, 4) * 3.1 + 0.4) * torch.cos(ys / max(h, 4) * 2.3)
    if nonpositive_block:
        d[: max(h // 3, 1), : max(w // 3, 1)] = 0.0
        d[0, 0] = -0.25
    if depth_column is not None:
        d[:, depth_column] = torch.tensor([DEPTH_COLUMN_VALUES[y % len(DEPTH_COLUMN_VALUES)] for y in range(h)], dtype=torch.float64)
    if collapse:
        fmap = torch.full_like(fmap, 2.0)
        d = torch.full_like(d, 1e4)
    if disp_range is not None:
        lo, hi = 1.0 / disp_range[1], 1.0 / disp_range[0]
        d = (d - lo) / (hi - lo)
        if depth_column is not None:
            d[:, depth_column] = torch.tensor([_raw_disparity(DEPTH_COLUMN_VALUES[y % len(DEPTH_COLUMN_VALUES)], disp_range) for y in range(h)],
                                              dtype=torch.float64)
    g3 = torch.Generator().manual_seed(seed * 104729 + 3)
    return dict(fmap=fmap, fmaps_ref=torch.stack(refs), inv_depth=d[None, None], K=K, ref_Ks=torch.stack(ref_Ks), poses=torch.stack(poses),
                g_mean=torch.rand(1, C, h, w, generator=g3, dtype=torch.float64) + 0.5, g_none=torch.rand(V, C, h, w, generator=g3, dtype=torch.float64) + 0.5)


INPUTS = ("fmap", "fmaps_ref", "inv_depth", "poses")
STRADDLE_DEPTH = 1.7          # inside the depths of a case, 1 / 0.65 .. 1 / 0.35
# The straddling camera sits INSIDE the scene: of the points in front of it only those in its frustum are sampled, and with the
# other views' focal length that is a cone of about two pixels' width.  A quarter of the focal length opens it to a tenth of the map.
STRADDLE_FOCAL = 0.25
LARGE_ANGLES = ((0.5, -0.4, 0.7), (-0.35, 0.6, -0.9), (0.8, 0.3, 0.25))


def run_warp_cost(route, case, dtype, device, decisions=None, need=INPUTS, reduce="mean", **opts):
    """`route` is "torch" (the restatement) or a callable with `fused_warp_cost`'s signature.  The loss is sum(cost * g_<reduce>).
    Returns a dict of detached results: cost, cells, g_fmap, g_fmaps_ref, g_inv_depth, g_poses (None where not in `need`), and for the
    restatement also coords and pz."""
    t = {k: v.detach().to(device=device, dtype=dtype).clone() for k, v in case.items()}
    for k in INPUTS:
        t[k].requires_grad_(k in need)
    args = (t["fmap"], t["fmaps_ref"], t["inv_depth"], t["K"], t["ref_Ks"], t["poses"])
    if route == "torch":
        out = warp_cost_reference(*args, reduce=reduce, decisions=decisions, **opts)
    else:
        cost, cells = route(*args, reduce=reduce, return_cells=True, **opts)
        out = dict(cost=cost, cells=cells)
    if need:
        (out["cost"] * t["g_" + reduce]).sum().backward()
    res = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    for k in INPUTS:
        res["g_" + k] = t[k].grad
    return res


def frame_masks(ref, h, w):
    """[V,h,w] booleans of a restatement's run: the samples with all four taps live (0 <= u < w - 1 and 0 <= v < h - 1), and those in
    the one-pixel border band, in frame with one or two live taps."""
    u, v = ref["coords"][:, 0], ref["coords"][:, 1]
    live4 = (u >= 0) & (u < w - 1) & (v >= 0) & (v < h - 1)
    return live4, (u > -1) & (u < w) & (v > -1) & (v < h) & ~live4


def near_border_share(ref64, ref32, h, w):
    """The share of (view, pixel) pairs of the float64 restatement whose u or v lies within 8 x the float32 coordinate error of an
    integer (while within that distance of the frame (-1, w) x (-1, h): beyond it no tap changes), or whose P.z lies within 8 x its
    float32 error of 1e-5.  The errors are measured: the largest |float32 - float64| over the pairs that are in frame."""
    c64, c32 = ref64["coords"].double(), ref32["coords"].double().to(ref64["coords"].device)
    u, v = c64[:, 0], c64[:, 1]
    inside = (u > -1) & (u < w) & (v > -1) & (v < h)
    e = float((c32 - c64).abs().amax(1)[inside].max()) if bool(inside.any()) else 0.0
    ez = float((ref32["pz"].double().to(c64.device) - ref64["pz"].double()).abs().max())
    m = 8 * e
    near = torch.zeros_like(inside)
    for c, size in ((u, w), (v, h)):
        near |= ((c - c.round()).abs() <= m) & (c >= -1 - m) & (c <= size + m)
    near &= (u >= -1 - m) & (u <= w + m) & (v >= -1 - m) & (v <= h + m)
    near |= (ref64["pz"].double() - 1e-5).abs() <= 8 * ez
    return float(near.double().mean()), e, ez
