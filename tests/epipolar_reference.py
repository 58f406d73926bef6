"""A torch restatement of GGRt's epipolar sampling stage: `EpipolarSampler.forward` (generate_image_rays, project_rays with near
and far given, the sample points, the bilinear gather from the OTHER views' feature maps, the validity mask) and the depth lines
of `EpipolarTransformer.forward` (get_depth, the clip to [near, far], depth_to_relative_disparity).  Our own text, dtype-generic:
it runs on the CPU in float64 (what the kernels are compared with) and on the device in float32 (the float32 torch route whose
error sets the bar).  It does not call torch.linalg.lstsq: the 3x3 normal system of intersect_rays is solved in closed form
(adjugate over determinant), which is the same solution wherever the rays are not parallel.

`make_case` draws seeded camera families and moves to the next seed until `margin_violations` is zero, so that `valid` can be
demanded equal on EVERY ray."""
import math

import torch
import torch.nn.functional as F

F32_EPS = float(torch.finfo(torch.float32).eps)   # project_camera_space's epsilon, whatever the dtype
MARGIN = 1e-4


def other_views(v, device="cpu"):
    """[v, v-1]: the view that (view, other_view) samples from, o = ov + (ov >= view)"""
    return torch.tensor([[ov + (ov >= i) for ov in range(v - 1)] for i in range(v)], dtype=torch.long, device=device)


def _in_bounds(x, y, probe):
    if probe is not None:
        for q in (x, y):
            probe.append((q, -1e-6, "point"))
            probe.append((q, 1 + 1e-6, "point"))
    return (x >= -1e-6) & (y >= -1e-6) & (x <= 1 + 1e-6) & (y <= 1 + 1e-6)


def _point_projection(K, O, D, t, probe):
    """the projection of O + t·D (camera space) with project_camera_space's epsilon and clamp"""
    P = O + t[..., None] * D
    p = P / (P[..., 2:] + F32_EPS)
    p = p.nan_to_num(nan=0.0, posinf=1e8, neginf=-1e8)
    x = K[..., 0, 0] * p[..., 0] + K[..., 0, 1] * p[..., 1] + K[..., 0, 2] * p[..., 2]
    y = K[..., 1, 0] * p[..., 0] + K[..., 1, 1] * p[..., 1] + K[..., 1, 2] * p[..., 2]
    if probe is not None:
        probe.append((P[..., 2], -1e-6, "point"))
    valid = _in_bounds(x, y, probe) & (P[..., 2] > -1e-6) & (t > -1e-6)
    return t.expand(valid.shape), x, y, valid


def _frame_intersection(K, O, D, dim, value, probe):
    """where the projected ray crosses the frame line `dim` = value"""
    od = 1 - dim
    fs, fo, cs, co = K[..., dim, dim], K[..., od, od], K[..., dim, 2], K[..., od, 2]
    os_, oo, ds, do, oz, dz = O[..., dim], O[..., od], D[..., dim], D[..., od], O[..., 2], D[..., 2]
    c = (value - cs) / fs
    t = (c * oz - os_) / (ds - c * dz)
    other = co + fo * (oo * (c * dz - ds) + do * (os_ - c * oz)) / (dz * os_ - ds * oz)
    same = torch.ones_like(other) * value
    z = oz + t * dz
    if probe is not None:
        probe.extend([(other, -1e-6, "frame"), (other, 1 + 1e-6, "frame"), (z, -1e-6, "frame"), (t, -1e-6, "frame")])
    ok = (other >= -1e-6) & (other <= 1 + 1e-6) & (z > -1e-6) & (t > -1e-6)      # (the fixed coordinate is in bounds exactly)
    x, y = (same, other) if dim == 0 else (other, same)
    return t, x, y, ok


def _reduce(cands, largest):
    """torch.min / torch.max over the candidates' t with the invalid ones pushed to the far end; the first index wins a tie"""
    lowest = -math.inf if largest else math.inf
    t = torch.stack([torch.where(ok, tt, torch.full_like(tt, lowest)) for tt, _, _, ok in cands])
    sel = (t.max(dim=0) if largest else t.min(dim=0)).indices[None]
    pick = lambda i: torch.stack([cand[i] for cand in cands]).gather(0, sel)[0]
    return pick(1), pick(2), pick(3)


def _world_rays(xy, c2w, Kinv):
    """get_world_rays: xy [..., 2] with c2w [..., 4, 4] and Kinv [..., 3, 3] broadcasting against it"""
    d = Kinv[..., :, 0] * xy[..., 0:1] + Kinv[..., :, 1] * xy[..., 1:2] + Kinv[..., :, 2]
    d = d / d.norm(dim=-1, keepdim=True)
    R = c2w[..., :3, :3]
    d = R[..., :, 0] * d[..., 0:1] + R[..., :, 1] * d[..., 1:2] + R[..., :, 2] * d[..., 2:3]
    return c2w[..., :3, 3].expand(d.shape), d


def _solve3(A, r):
    """A x = r for symmetric-or-not 3x3 A [..., 3, 3], by the adjugate"""
    a, b, c, d, e, f, g, h, i = (A[..., j, k] for j in range(3) for k in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * c00 + b * c10 + c * c20
    x = (c00 * r[..., 0] + c01 * r[..., 1] + c02 * r[..., 2]) / det
    y = (c10 * r[..., 0] + c11 * r[..., 1] + c12 * r[..., 2]) / det
    z = (c20 * r[..., 0] + c21 * r[..., 1] + c22 * r[..., 2]) / det
    return torch.stack([x, y, z], dim=-1)


def _intersect(ox, dx, oy, dy, probe):
    """intersect_rays: the least-squares point of two rays, 1e10 where they are parallel"""
    dot = (dx * dy).sum(-1)
    if probe is not None:
        probe.append((dot, 1 - 1e-5, "dot"))
    eye = torch.eye(3, dtype=ox.dtype, device=ox.device)
    nx = dx[..., :, None] * dx[..., None, :] - eye
    ny = dy[..., :, None] * dy[..., None, :] - eye
    rhs = (nx * ox[..., None, :]).sum(-1) + (ny * oy[..., None, :]).sum(-1)
    p = _solve3(nx + ny, rhs)
    return torch.where((dot > 1 - 1e-5)[..., None], torch.full_like(p, 1e10), p)


def epipolar_reference(images, extrinsics, intrinsics, near, far, num_samples, ray_window=None, probe=None, details=False):
    """images [b,v,c,h,w], extrinsics [b,v,4,4] (camera to world), intrinsics [b,v,3,3] (normalised), near / far [b,v].
    Returns a dict with the fields of the reference's EpipolarSampling plus `depth` (the relative disparity that goes into the
    depth encoding); `details` adds the raw clipped depth and the two branch flags of project_rays."""
    b, v, c, h, w = images.shape
    dt, dev = images.dtype, images.device
    s = int(num_samples)
    ys, xs = (torch.arange(h, device=dev).to(dt) + 0.5) / h, (torch.arange(w, device=dev).to(dt) + 0.5) / w
    if ray_window is not None:
        y0, y1, x0, x1 = ray_window
        ys, xs = ys[y0:y1], xs[x0:x1]
    xy = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), dim=-1).reshape(-1, 2)     # [r, 2], x fastest
    Kinv = torch.linalg.inv(intrinsics)
    origins, directions = _world_rays(xy, extrinsics[:, :, None], Kinv[:, :, None])                 # [b, v, r, 3]

    idx = other_views(v, dev)
    c2w_o, K_o, Kinv_o = extrinsics[:, idx], intrinsics[:, idx], Kinv[:, idx]                          # [b, v, ov, ...]
    w2c_o = torch.linalg.inv(c2w_o)[:, :, :, None]                                                     # [b, v, ov, 1, 4, 4]
    K4 = K_o[:, :, :, None]
    og, dg = origins[:, :, None], directions[:, :, None]                                               # [b, v, 1, r, 3]
    Rw = w2c_o[..., :3, :3]
    O = Rw[..., :, 0] * og[..., 0:1] + Rw[..., :, 1] * og[..., 1:2] + Rw[..., :, 2] * og[..., 2:3] + w2c_o[..., :3, 3]
    D = Rw[..., :, 0] * dg[..., 0:1] + Rw[..., :, 1] * dg[..., 1:2] + Rw[..., :, 2] * dg[..., 2:3]

    frame = [_frame_intersection(K4, O, D, dim, value, probe) for dim, value in ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0))]
    fmin, fmax = _reduce(frame, False), _reduce(frame, True)
    _, nx, ny, nok = _point_projection(K4, O, D, near[:, :, None, None], probe)
    _, fx, fy, fok = _point_projection(K4, O, D, far[:, :, None, None], probe)
    min_x, min_y, min_ok = torch.where(nok, nx, fmin[0]), torch.where(nok, ny, fmin[1]), torch.where(nok, nok, fmin[2])
    max_x, max_y, max_ok = torch.where(fok, fx, fmax[0]), torch.where(fok, fy, fmax[1]), torch.where(fok, fok, fmax[2])
    valid = min_ok & max_ok                                                                            # [b, v, ov, r]
    clean = lambda x, y: torch.stack([x, y], dim=-1).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0) * valid[..., None]
    xy_min, xy_max = clean(min_x, min_y)[..., None, :], clean(max_x, max_y)[..., None, :]             # [b, v, ov, r, 1, 2]
    pos = ((torch.arange(s, device=dev).to(dt) + 0.5) / s)[:, None]
    half = 0.5 / s
    xy_sample = xy_min + pos * (xy_max - xy_min)                                                       # [b, v, ov, r, s, 2]
    r = xy.shape[0]

    maps = images[:, idx].reshape(b * v * (v - 1), c, h, w)
    got = F.grid_sample(maps, (2 * xy_sample - 1).reshape(b * v * (v - 1), r, s, 2), mode="bilinear", padding_mode="zeros",
                        align_corners=False)
    features = got.reshape(b, v, v - 1, c, r, s).permute(0, 1, 2, 4, 5, 3) * valid[..., None, None]

    oy, dy = _world_rays(xy_sample.detach(), c2w_o[:, :, :, None, None], Kinv_o[:, :, :, None, None])
    ox, dx = origins[:, :, None, :, None], directions[:, :, None, :, None]
    point = _intersect(ox.expand(oy.shape), dx.expand(oy.shape), oy, dy, probe)
    raw = (point - ox).norm(dim=-1)
    nr, fr = near[:, :, None, None, None], far[:, :, None, None, None]
    clipped = raw.maximum(nr).minimum(fr)
    dn, df = 1 / (nr + 1e-10), 1 / (fr + 1e-10)
    depth = 1 - (1 / (clipped + 1e-10) - df) / (dn - df + 1e-10)

    out = dict(features=features, valid=valid, xy_ray=xy.expand(b, v, r, 2), xy_sample=xy_sample,
               xy_sample_near=xy_min + (pos - half) * (xy_max - xy_min), xy_sample_far=xy_min + (pos + half) * (xy_max - xy_min),
               origins=origins, directions=directions, depth=depth)
    if details:
        out.update(raw_depth=clipped, min_valid=nok, max_valid=fok, near_xy=torch.stack([nx, ny], -1), far_xy=torch.stack([fx, fy], -1),
                   near_z=(O + nr * D)[..., 2], far_z=(O + fr * D)[..., 2], dot=(dx * dy).sum(-1))
    return out


FLOAT_OUTPUTS = ("features", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions", "depth")
CASE_ARGS = ("images", "extrinsics", "intrinsics", "near", "far", "num_samples", "ray_window")


def margin_violations(case):
    """The number of places where `case` breaks the margin rule: a validity quantity of any ray (an xy component of one of the
    six projections against 0 − 1e-6 and 1 + 1e-6, a camera-space z or a t against −1e-6) within 1e-4 of its threshold, a
    direction dot product within 1e-4 of 1 − 1e-5, or a ray whose `valid` differs between the float32 and the float64 run.

    A case may carry `shared_centre`, bool [v, v-1]: the (view, other view) pairs whose two cameras stand at the same point, which
    only the "rotation" family sets.  On those pairs, and on no others, two entries are left out: the frame-intersection
    quantities (the casting origin is the sampled camera's centre, so t = 0/x and z = 0 exactly and `other` = 0/0 = NaN in
    every precision: such a hit is refused whatever its t) and the dot product of their VALID rays (it is 1 up to rounding, on
    the parallel side of the threshold by 1e-5; the test that uses the family asserts its own bound on it).  The point
    projections, the dot products of invalid rays and the float32 / float64 comparison of `valid` stay."""
    args = {k: case[k] for k in CASE_ARGS}
    shared = case.get("shared_centre")
    probe = []
    with torch.no_grad():
        ref = epipolar_reference(**args, probe=probe)
        low = epipolar_reference(**{k: (a.float() if torch.is_tensor(a) else a) for k, a in args.items()})
    count = 0
    for q, thr, kind in probe:
        close = (q - thr).abs() < MARGIN
        if shared is not None and kind != "point":
            skip = shared[None, :, :, None].expand(ref["valid"].shape)
            close = close & ~((skip & ref["valid"])[..., None] if kind == "dot" else skip)
        count += int(close.sum())
    return count + int((ref["valid"] != low["valid"]).sum())


def _look_at_z(yaw, pitch, position):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    rx = torch.tensor([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=torch.float64)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = ry @ rx
    m[:3, 3] = torch.as_tensor(position, dtype=torch.float64)
    return m


# family: (yaw amplitude, baseline, near, far).  "default" is the family the sampler was first tried with; "inside" keeps most
# segments wholly inside the other frame (near / far branches), "clipped" cuts most of them at the frame (frame-intersection
# branches), "away" turns the views' backs to each other (nothing valid), "nearfar" gives every view its own near = far / 2.
# "rotation": views 0 and 1 stand at the origin EXACTLY and differ by a yaw and a pitch of a few hundredths of a radian, so every
# sample's ray of one is parallel to the casting ray of the other (intersect_rays' parallel branch); view 1's focal lengths are
# about 0.6 against view 0's 0.9 … 1.1, so view 0's whole frame projects inside view 1 (segments from the near and far
# projections; the frame intersections are 0/0 at a shared centre and are never consulted there).  Views 2 … are displaced as in
# "default": parallel and non-parallel pairs in one call.
FAMILIES = {"default": (0.15, 0.4, 1.0, 20.0), "inside": (0.066, 0.4, 2.0, 4.0), "clipped": (0.45, 1.2, 0.2, 100.0),
            "away": (0.0, 0.4, 1.0, 20.0), "nearfar": (0.12, 0.4, None, None), "rotation": (0.15, 0.4, 1.0, 20.0)}


def _draw(b, v, h, w, c, s, seed, family, window):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1
    yaw, baseline, near, far = FAMILIES[family]
    ext = torch.empty(b, v, 4, 4, dtype=torch.float64)
    K = torch.zeros(b, v, 3, 3, dtype=torch.float64)
    for i in range(b):
        for j in range(v):
            side = (j - (v - 1) / 2) / max((v - 1) / 2, 1)                   # −1 … 1 across the views
            jitter = rnd(5)
            if family == "away":
                angle = math.pi * j + (math.pi / 2 if j >= 2 else 0.0) + 0.05 * float(jitter[0])
                if v > 2:
                    angle = 2 * math.pi * j / v + 0.05 * float(jitter[0])
                pos = (0.3 * math.sin(angle), 0.0, 0.3 * math.cos(angle))     # each camera looks outwards from a small circle
                ext[i, j] = _look_at_z(angle, 0.02 * float(jitter[1]), pos)
            elif family == "rotation" and j < 2:
                turn = (0.03 + 0.01 * float(jitter[0])) * (1 if j == 0 else -1)
                ext[i, j] = _look_at_z(turn, 0.03 * float(jitter[1]), (0.0, 0.0, 0.0))
            else:
                pos = (side * baseline + 0.05 * baseline * float(jitter[2]), 0.1 * baseline * float(jitter[3]), 0.05 * baseline * float(jitter[4]))
                ext[i, j] = _look_at_z(-side * yaw + 0.03 * float(jitter[0]), 0.05 * float(jitter[1]), pos)
            k = rnd(4)
            K[i, j] = torch.tensor([[0.9 + 0.1 * float(k[0]), 0, 0.5 + 0.02 * float(k[1])], [0, 1.1 + 0.1 * float(k[2]), 0.5 + 0.02 * float(k[3])],
                                    [0, 0, 1]], dtype=torch.float64)
            if family == "rotation" and j == 1:
                K[i, j, 0, 0], K[i, j, 1, 1] = 0.6 + 0.02 * float(k[0]), 0.6 + 0.02 * float(k[2])
    if family == "nearfar":
        far_t = 8.0 + 4.0 * torch.arange(b * v, dtype=torch.float64).reshape(b, v) + rnd(b, v)
        near_t = far_t / 2
    else:
        near_t = near * (1 + 0.05 * rnd(b, v))
        far_t = far * (1 + 0.05 * rnd(b, v))
    images = torch.randn(b, v, c, h, w, generator=gen, dtype=torch.float64)
    case = dict(images=images, extrinsics=ext, intrinsics=K, near=near_t, far=far_t, num_samples=s, ray_window=window)
    if family == "rotation":
        idx = other_views(v)
        case["shared_centre"] = (torch.arange(v)[:, None] < 2) & (idx < 2)
    return case


def make_case(b, v, h, w, c, s, seed, family="default", window=None, tries=4000):
    """The first admissible case at or after `seed` (the seed moves on until `margin_violations` is zero).  The margin rule is
    about cameras and rays only, so it is searched with one channel and the images are drawn afterwards."""
    for k in range(tries):
        probe_case = _draw(b, v, h, w, 1, s, seed + k, family, window)
        if margin_violations(probe_case) == 0:
            case = _draw(b, v, h, w, c, s, seed + k, family, window)
            case["seed"] = seed + k
            return case
    raise RuntimeError(f"no admissible case in {tries} seeds from {seed} ({family}, v={v}, {h}x{w})")


def run_case(fn, case, dtype=torch.float64, device="cpu", **more):
    args = {k: (case[k].to(device=device, dtype=dtype) if torch.is_tensor(case[k]) else case[k]) for k in CASE_ARGS}
    return fn(**args, **more)
