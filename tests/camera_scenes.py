"""Scenes OFF the camera family of `synthetic.make_scene` (60° field of view, square pixels, centred principal point, means
inside the frame + 5 %, view depth in [1.5, 50], unit quaternions, scale_modifier 1), one named constructor per property, and
each constructor ASSERTS on the C oracle's forward state that its scene has the property (tests/test_camera_scenes_reference.py
runs them without a GPU; tests/test_gpu_camera_family.py holds the kernels to the references on them).

A scene starts from `make_scene` under the identity pose (camera frame = world frame), is stretched into the requested frustum,
gets its groups of Gaussians moved in the CAMERA frame — beyond the frustum clamp 1.3·tan(fov/2), in front of / behind the near
cull 0.2 — and is then carried into the world by the pose.  `CameraScene.groups` names the Gaussians each property placed.

Plain module, not a test file (like tests/sort_scenes.py)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from ggrt_official_amd.synthetic import Scene, camera_matrices, make_scene
from oracle import torch_raster as tr
from tests.helpers import FWD_ATOL, oracle_forward

CLAMP, NEAR = 1.3, 0.2                      # restated on purpose: a changed constant in the product must fail a claim here
NEAR32 = np.float32(NEAR)


@dataclass
class CameraScene:
    name: str
    sc: Scene
    scale_modifier: float = 1.0
    fov_deg: float = 60.0
    cx: float = 0.5
    cy: float = 0.5
    groups: dict = field(default_factory=dict)        # name -> bool [P]

    def settings(self, **kw):
        return self.sc.settings()._replace(scale_modifier=self.scale_modifier, **kw)


# ---- camera ---------------------------------------------------------------------------------------------------------------------
def camera(W, H, fov_deg=60.0, aspect=1.0, cx=0.5, cy=0.5, c2w=None, near=1.0, far=100.0):
    """`camera_matrices` with tan(fov_y/2) = `aspect` × the square-pixel value: (view, full, campos, tanfovx, tanfovy), the two
    tangents rounded to float32 (what every consumer holds them in)."""
    view, full, campos, tanfovx, tanfovy, _, _ = camera_matrices(W, H, fov_deg, near, far, c2w, cx, cy)
    if aspect != 1.0:
        tanfovy = tanfovy * aspect
        Pm = torch.zeros(4, 4, dtype=torch.float64)
        Pm[0, 0], Pm[1, 1] = near / tanfovx, near / tanfovy
        Pm[0, 2], Pm[1, 2], Pm[3, 2] = 2 * cx - 1, 2 * cy - 1, 1
        Pm[2, 2], Pm[2, 3] = far / (far - near), -(far * near) / (far - near)
        c2w64 = torch.eye(4, dtype=torch.float64) if c2w is None else c2w.double()
        full = (torch.linalg.inv(c2w64).T @ Pm.T).float()
    return view, full, campos, float(np.float32(tanfovx)), float(np.float32(tanfovy))


def pose(seed, angle=0.3, shift=0.5):
    """a rotated and translated camera-to-world pose (float64)"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * angle
    K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = torch.matrix_exp(K)
    T[:3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * shift
    return T


def cov6_of(scales, rotations, mod=1.0):
    """[P,6] of (mod·scales, rotations AS GIVEN: upstream does not normalise the quaternion) in float64"""
    return tr.cov3d_from_scale_rot(scales.double(), rotations.double(), mod)


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def build(name, P, W, H, D=3, seed=0, fov_deg=60.0, aspect=1.0, cx=0.5, cy=0.5, c2w=None, clamp=0.0, near=0.0, on_cull=0,
          quat_norms=None, scale_modifier=1.0, profile="A") -> CameraScene:
    """`clamp`, `near`: the fractions of the Gaussians moved beyond the frustum clamp / around the near cull; `on_cull`: the
    number of Gaussians put on each of the three depths 0.2, next float above, next float below (identity pose only)."""
    base = make_scene(P, W, H, sh_degree=D, profile=profile, seed=seed)            # identity pose, the 60° family
    view, full, campos, tanfovx, tanfovy = camera(W, H, fov_deg, aspect, cx, cy, c2w)
    rng = np.random.default_rng(7000 + seed)
    m = base.means3D.double().numpy().copy()
    s = base.scales.double().numpy().copy()
    op = base.opacities.double().numpy().copy()
    kx, ky = tanfovx / base.tanfovx, tanfovy / base.tanfovy
    z = m[:, 2].copy()
    rx = m[:, 0] / z * kx + (1 - 2 * cx) * tanfovx                                  # x/z, y/z: the frame of THIS camera + 5 %
    ry = m[:, 1] / z * ky + (1 - 2 * cy) * tanfovy
    s *= math.sqrt(kx * ky)                                                         # footprints in pixels stay what they were
    order = rng.permutation(P)
    groups, taken = {}, 0

    def take(n):
        nonlocal taken
        ids = order[taken:taken + n]
        taken += n
        return ids

    if on_cull:
        assert c2w is None, "the exact depths need the identity pose"
        for tag, zz in (("at_cull", NEAR32), ("above_cull", np.nextafter(NEAR32, np.float32(1))),
                                       ("below_cull", np.nextafter(NEAR32, np.float32(0)))):
            ids = take(on_cull)
            s[ids] *= (float(zz) / z[ids])[:, None]
            z[ids] = float(zz)
            groups[tag] = ids
    if near:
        ids = take(int(near * P))
        zn = rng.uniform(0.12, 0.40, len(ids))
        huge = ids[:min(len(ids) // 10, 64)]      # keep their world size: hundreds of pixels wide, radii beyond 1 000 px …
        rest = ids[len(huge):]
        s[rest] *= (zn[len(huge):] / z[rest])[:, None]
        op[huge] *= 0.2                           # … and faint, so that they do not hide the frame behind them
        z[ids] = zn
        groups["near"] = ids
    if clamp:
        ids = take(int(clamp * P))
        kind = np.arange(len(ids)) % 3            # x only, y only, both
        sign = lambda n: np.where(rng.random(n) < 0.5, -1.0, 1.0)
        out = lambda n: rng.uniform(1.36, 2.4, n)
        gx_, gy_ = ids[kind != 1], ids[kind != 0]
        rx[gx_] = sign(len(gx_)) * out(len(gx_)) * tanfovx
        ry[gy_] = sign(len(gy_)) * out(len(gy_)) * tanfovy
        keep_in = lambda r, t: np.clip(r, -0.95 * t, 0.95 * t)
        rx[ids[kind == 1]] = keep_in(rx[ids[kind == 1]], tanfovx)
        ry[ids[kind == 0]] = keep_in(ry[ids[kind == 0]], tanfovy)
        s[ids] *= 6.0 * max(W, H) / 112.0         # large enough to reach into the frame from out there
        groups["clamp"] = ids
    cam = np.stack([rx * z, ry * z, z], -1)
    q = base.rotations.double()
    if quat_norms is not None:
        q = q * torch.from_numpy(rng.uniform(quat_norms[0], quat_norms[1], P))[:, None]
        groups["quat_norm"] = q.norm(dim=-1).numpy()
    pts = torch.from_numpy(cam)
    if c2w is not None:
        pts = pts @ c2w.double()[:3, :3].T + c2w.double()[:3, 3]
    elif on_cull:
        pts = pts.clone()
        for tag in ("at_cull", "above_cull", "below_cull"):                         # the float32 depth, bit for bit
            pts[groups[tag], 2] = float(np.float32(z[groups[tag]][0]))
    scales = torch.from_numpy(s)
    sc = Scene(means3D=pts.float(), cov3D=cov6_of(scales.float(), q.float(), scale_modifier).float(), scales=scales.float(),
               rotations=q.float(), opacities=torch.from_numpy(op).float(), shs=base.shs, viewmatrix=view, projmatrix=full,
               campos=campos, bg=torch.zeros(3), tanfovx=tanfovx, tanfovy=tanfovy, width=W, height=H, sh_degree=D)
    masks = {}
    for k, v in groups.items():
        if k == "quat_norm":
            masks[k] = v
        else:
            masks[k] = np.zeros(P, bool)
            masks[k][v] = True
    return CameraScene(name=name, sc=sc, scale_modifier=scale_modifier, fov_deg=fov_deg, cx=cx, cy=cy, groups=masks)


# ---- what the oracle says about a scene ---------------------------------------------------------------------------------------
def oracle_state(cs: CameraScene, use_sh=True, use_cov=False, colors=None, sh_cap=3, tight=True):
    """The C oracle's forward of the scene, with ITS scale_modifier (the scale + rotation inputs by default)."""
    return oracle_forward(cs.sc, use_sh=use_sh, use_cov=use_cov, colors=colors, sh_cap=sh_cap, tight=tight,
                          scale_modifier=cs.scale_modifier)


def view_space(cs: CameraScene):
    """(x/z, y/z, z) per Gaussian in float32, the oracle's operation order"""
    m, V = cs.sc.means3D.numpy(), cs.sc.viewmatrix.numpy().reshape(16)
    t = [m[:, 0] * V[k] + m[:, 1] * V[4 + k] + m[:, 2] * V[8 + k] + V[12 + k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return t[0] / t[2], t[1] / t[2], t[2]


def clamp_classes(cs: CameraScene, st):
    """bool [P] per class: visible with tiles, and beyond 1.3·tanfov (by a clear margin) in x only / y only / both"""
    rx, ry, z = view_space(cs)
    seen = (st.radii > 0) & (st.tiles_touched > 0)
    bx = np.abs(rx) > CLAMP * cs.sc.tanfovx * 1.001
    by = np.abs(ry) > CLAMP * cs.sc.tanfovy * 1.001
    ix = np.abs(rx) < CLAMP * cs.sc.tanfovx * 0.999
    iy = np.abs(ry) < CLAMP * cs.sc.tanfovy * 0.999
    return dict(x_only=seen & bx & iy, y_only=seen & by & ix, both=seen & bx & by), rx, ry


def assert_clamp(cs: CameraScene, st=None):
    st = st or oracle_state(cs)
    cls, rx, ry = clamp_classes(cs, st)
    P = st.P
    total = sum(int(c.sum()) for c in cls.values())
    assert total >= 0.05 * P, f"{cs.name}: only {total} of {P} Gaussians are visible beyond the frustum clamp"
    for k, c in cls.items():
        for axis, r in (("x", rx), ("y", ry)):
            if k in (axis + "_only", "both"):
                assert (c & (r > 0)).sum() >= 3 and (c & (r < 0)).sum() >= 3, f"{cs.name}: class {k} lacks a sign of {axis}"
    return st


def assert_near(cs: CameraScene, st=None):
    st = st or oracle_state(cs)
    _, _, z = view_space(cs)
    P = st.P
    front = (z > NEAR32) & (z < 0.4) & (st.radii > 0)
    behind = (z > 0.1) & (z <= NEAR32)
    assert front.sum() >= 0.05 * P, f"{cs.name}: {int(front.sum())} of {P} visible with 0.2 < z < 0.4"
    assert behind.sum() >= 0.02 * P and not st.radii[behind].any(), f"{cs.name}: {int(behind.sum())} culled in (0.1, 0.2]"
    assert st.radii.max() > 1000, f"{cs.name}: largest radius {st.radii.max()} px"
    # some of them contribute: without them the image is another one
    hidden = copy_scene(cs, opacities=torch.where(torch.from_numpy(front)[:, None], torch.zeros_like(cs.sc.opacities),
                                                  cs.sc.opacities))
    changed = np.abs(oracle_state(hidden).color - st.color).max(0) > 1e-3
    assert changed.mean() > 0.25, f"{cs.name}: the near Gaussians move {changed.mean():.1%} of the pixels"
    return st


def assert_on_cull(cs: CameraScene, st=None):
    st = st or oracle_state(cs)
    z = cs.sc.means3D[:, 2].numpy()
    g = cs.groups
    assert (z[g["at_cull"]] == NEAR32).all() and (z[g["above_cull"]] == np.nextafter(NEAR32, np.float32(1))).all()
    assert (z[g["below_cull"]] == np.nextafter(NEAR32, np.float32(0))).all()
    assert np.array_equal(view_space(cs)[2], z), "the identity pose must leave the depth bits alone"
    assert not st.radii[g["at_cull"]].any() and not st.radii[g["below_cull"]].any(), "culled at and below 0.2"
    assert (st.radii[g["above_cull"]] > 0).mean() > 0.9, "kept on the next float above 0.2"
    assert (st.depth[g["above_cull"]][st.radii[g["above_cull"]] > 0] == np.nextafter(NEAR32, np.float32(1))).all()
    return st


def assert_camera(cs: CameraScene, st=None):
    """Gaussian 0 sits on the optical axis: it lands on the principal point, several pixels off the frame's centre."""
    st = st or oracle_state(cs)
    sc = cs.sc
    W, H = sc.width, sc.height
    assert W % 16 and H % 16
    assert cs.fov_deg in (25.0, 60.0, 100.0) and abs(sc.tanfovx - math.tan(math.radians(cs.fov_deg) / 2)) < 1e-6
    fx, fy = W / (2 * sc.tanfovx), H / (2 * sc.tanfovy)
    assert abs(fx / fy - 1) > 0.05, "pixels are square"
    assert st.radii[0] > 0
    want = np.array([cs.cx * W - 0.5, cs.cy * H - 0.5])
    assert np.abs(st.xy[0] - want).max() < 1e-3, (st.xy[0], want)
    assert np.abs(want - np.array([(W - 1) / 2, (H - 1) / 2])).min() >= 3.0, "principal point within 3 px of the centre"
    assert (st.radii > 0).mean() > 0.5, "the scene does not fill this camera's frame"
    return st


def assert_modifier(cs: CameraScene, st=None):
    st = st or oracle_state(cs)
    assert cs.scale_modifier in (0.6, 1.7)
    n = cs.groups["quat_norm"]
    assert n.min() >= 0.7 and n.max() <= 1.3 and n.min() < 0.75 and n.max() > 1.25
    sc = cs.sc
    assert np.abs(sc.rotations.norm(dim=-1).numpy() - n).max() < 1e-6
    want = cov6_of(sc.scales, sc.rotations, cs.scale_modifier).numpy()           # the quaternion as given
    unit = cov6_of(sc.scales, sc.rotations / sc.rotations.norm(dim=-1, keepdim=True), cs.scale_modifier).numpy()
    scale = np.abs(want).max(1, keepdims=True)
    assert (np.abs(st.cov3D - want) / scale).max() < 1e-5, "the oracle's covariance is not that of (modifier·scale, raw quaternion)"
    assert (np.abs(st.cov3D - unit) / scale).max() > 0.1, "a normalised quaternion would give the same covariance"
    return st


# ---- the named constructors (each asserts its property on the C oracle) ----------------------------------------------------
def _axis_gaussian(cs: CameraScene):
    """Gaussian 0 onto the optical axis, 5 units ahead (camera frame: the pose carries it)"""
    sc = cs.sc
    c2w = torch.linalg.inv(sc.viewmatrix.double().T)
    sc.means3D[0] = (c2w[:3, :3] @ torch.tensor([0.0, 0.0, 5.0], dtype=torch.float64) + c2w[:3, 3]).float()
    return cs


def clamp_scene(P=3000, W=112, H=80, D=2, seed=0, **kw):
    cs = build("clamp", P, W, H, D, seed, clamp=0.25, **kw)
    assert_clamp(cs)
    return cs


def near_scene(P=3000, W=112, H=80, D=2, seed=0, **kw):
    cs = build("near", P, W, H, D, seed, near=0.125, **kw)
    assert_near(cs)
    return cs


def on_cull_scene(P=2000, W=112, H=80, D=2, seed=0, n=256):
    cs = build("on_cull", P, W, H, D, seed, on_cull=n)
    assert_on_cull(cs)
    return cs


def camera_scene(P=3000, W=118, H=84, D=2, seed=0, fov_deg=100.0, aspect=1.23, cx=0.42, cy=0.57, **kw):
    cs = _axis_gaussian(build("camera", P, W, H, D, seed, fov_deg=fov_deg, aspect=aspect, cx=cx, cy=cy, **kw))
    assert_camera(cs)
    return cs


def modifier_scene(P=3000, W=112, H=80, D=2, seed=0, scale_modifier=1.7, **kw):
    cs = build("modifier", P, W, H, D, seed, quat_norms=(0.7, 1.3), scale_modifier=scale_modifier, **kw)
    assert_modifier(cs)
    return cs


def mixed_scene(P=3000, W=118, H=84, D=2, seed=0, fov_deg=100.0, aspect=1.23, cx=0.42, cy=0.57, scale_modifier=1.7, c2w=None,
                **kw):
    """clamp + near + camera + modifier under a rotated and translated pose"""
    c2w = pose(seed + 10) if c2w is None else c2w
    cs = _axis_gaussian(build("mixed", P, W, H, D, seed, fov_deg=fov_deg, aspect=aspect, cx=cx, cy=cy, c2w=c2w, clamp=0.25,
                              near=0.125, quat_norms=(0.7, 1.3), scale_modifier=scale_modifier, **kw))
    assert not torch.equal(cs.sc.viewmatrix, torch.eye(4))
    st = oracle_state(cs)
    for check in (assert_clamp, assert_near, assert_camera, assert_modifier):
        check(cs, st)
    return cs


CONSTRUCTORS = dict(clamp=clamp_scene, near=near_scene, on_cull=on_cull_scene, camera=camera_scene, modifier=modifier_scene,
                    mixed=mixed_scene)


# ---- the torch reference on a scene -------------------------------------------------------------------------------------------
def torch_run(cs: CameraScene, dL, dLd=None, dtype=torch.float32, use_sh=True, use_cov=False, colors=None, pose=False, sh_cap=3,
              tile_filter=None, rasterize=None, **extra):
    """Forward + autograd backward of `oracle.torch_raster` in `dtype`: dict(color, radii, depth, grads, point_list, ranges,
    num_rendered).  `rasterize`: a composed reference with tr.rasterize's leading arguments (tests/aa_reference.py, …)."""
    sc = cs.sc
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    leaves = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities))
    kw = {}
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(sc.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(colors)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(sc.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(sc.scales)
        leaves["rotations"] = kw["rotations"] = leaf(sc.rotations)
    V, PM, cam = sc.viewmatrix.to(dtype), sc.projmatrix.to(dtype), sc.campos.to(dtype)
    if pose:
        V, PM, cam = leaf(V), leaf(PM), leaf(cam)
        leaves.update(viewmatrix=V, projmatrix=PM, campos=cam)
    args = (leaves["means3D"], leaves["opacities"], V, PM, cam, sc.bg, sc.width, sc.height, sc.tanfovx, sc.tanfovy, sc.sh_degree)
    if rasterize is not None:
        return leaves, rasterize(*args, sh_cap=sh_cap, **kw, **extra)
    color, radii, depth, state = tr.rasterize(*args, scale_modifier=cs.scale_modifier, return_state=True, sh_cap=sh_cap,
                                              depth_grad=dLd is not None, tile_filter=tile_filter, **kw)
    loss = (color * dL.to(dtype)).sum()
    if dLd is not None:
        loss = loss + (depth * dLd.to(dtype)).sum()
    loss.backward()
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in leaves.items()}
    return dict(color=color.detach().numpy(), radii=radii.numpy(), depth=depth.detach().numpy(), grads=grads,
                point_list=state["point_list"].numpy(), ranges=state["ranges"].numpy(), num_rendered=state["num_rendered"])


def flip_free(a, b, atol=FWD_ATOL, order=True):
    """two torch_run results made the same discrete decisions: equal radii and lists, images within the forward tolerance.
    `order=False`: the same Gaussians tile by tile, in whatever depth order (see POSE_CASES["large"])."""
    if not (np.array_equal(a["radii"], b["radii"]) and np.array_equal(a["ranges"], b["ranges"])
            and float(np.abs(a["color"] - b["color"]).max()) <= atol):
        return False
    if order:
        return np.array_equal(a["point_list"], b["point_list"])
    tile = np.repeat(np.arange(len(a["ranges"])), a["ranges"][:, 1] - a["ranges"][:, 0]).astype(np.int64) << 32
    return np.array_equal(np.sort(tile | a["point_list"]), np.sort(tile | b["point_list"]))


def copy_scene(cs: CameraScene, **fields) -> CameraScene:
    """A copy whose tensors are its own (in-place edits cannot reach the original), with `fields` of the Scene replaced."""
    d = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in cs.sc.__dict__.items()}
    d.update(fields)
    return CameraScene(cs.name, Scene(**d), cs.scale_modifier, cs.fov_deg, cs.cx, cs.cy, cs.groups)


# ---- the camera-gradient cases of tests/test_gpu_camera_family.py ------------------------------------------------------------
def large_scene(P=200_000, W=250, H=186, D=1, seed=0):
    """The mixed scene's camera, pose, modifier and quaternions at P >= 200 000 (the camera-gradient kernels reduce one partial
    per block of 256 Gaussians: hundreds of them), with smaller shares beyond the clamp and at the near plane so that the lists
    stay affordable for the torch reference on a SAMPLE of tiles."""
    cs = build("large", P, W, H, D, seed, fov_deg=100.0, aspect=1.23, cx=0.42, cy=0.57, c2w=pose(seed + 10), clamp=0.03,
               near=0.02, quat_norms=(0.7, 1.3), scale_modifier=1.7)
    st = oracle_state(cs)
    cls, _, _ = clamp_classes(cs, st)
    z = view_space(cs)[2]
    assert all(int(c.sum()) >= 300 for c in cls.values()), {k: int(c.sum()) for k, c in cls.items()}
    assert ((z > NEAR32) & (z < 0.4) & (st.radii > 0)).sum() >= 1000 and ((z > 0.1) & (z <= NEAR32)).sum() >= 500
    return cs


def tile_sample(W, H, stride):
    """(tile_filter, bool [H, W] mask) of every `stride`-th tile of the frame — the sampler of tests/test_gpu_full_size_vs_torch.py"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    mask = torch.zeros(H, W, dtype=torch.bool)
    for t in range(0, gx * gy, stride):
        mask[(t // gx) * 16:(t // gx + 1) * 16, (t % gx) * 16:(t % gx + 1) * 16] = True
    return (lambda tx, ty: (ty * gx + tx) % stride == 0), mask


# rel-L2 between the fp32 and the fp64 run of the torch reference (autograd, `pose=True`) on each case, measured on the CPU
# on a flip-free seed (equal radii and lists, images within FWD_ATOL): the references' own spread.  The GPU bar of a case is
# 10 × the largest of its three camera figures (one order, as the bars of tests/helpers.py), for means3D as well.
# tests/test_camera_scenes_reference.py measures them again and fails if a figure here understates the spread.
# `stride`: the torch leg blends every stride-th tile only, the upstream gradient is zero elsewhere on BOTH sides.
_CLAMP = lambda: clamp_scene(3000, 112, 80, 3, 0, c2w=pose(10))
_NEAR = lambda: near_scene(3000, 112, 80, 2, 0, c2w=pose(10))
_MIXED = lambda: mixed_scene(3000, 118, 84, 3, 0)
POSE_CASES = {
    "clamp": dict(make=_CLAMP, with_depth=False,
                  spread=dict(viewmatrix=1.70e-6, projmatrix=2.66e-6, campos=6.97e-7, means3D=2.86e-6)),
    "clamp+depth": dict(make=_CLAMP, with_depth=True,
                        spread=dict(viewmatrix=6.25e-7, projmatrix=3.15e-6, campos=6.97e-7, means3D=2.88e-6)),
    "near": dict(make=_NEAR, with_depth=False,
                 spread=dict(viewmatrix=6.84e-7, projmatrix=1.92e-6, campos=1.93e-6, means3D=2.76e-6)),
    "near+depth": dict(make=_NEAR, with_depth=True,
                       spread=dict(viewmatrix=5.32e-7, projmatrix=1.73e-6, campos=1.93e-6, means3D=2.71e-6)),
    "mixed": dict(make=_MIXED, with_depth=False,
                  spread=dict(viewmatrix=1.23e-6, projmatrix=3.46e-6, campos=3.81e-7, means3D=1.73e-6)),
    "mixed+depth": dict(make=_MIXED, with_depth=True,
                        spread=dict(viewmatrix=8.97e-7, projmatrix=3.58e-6, campos=3.81e-7, means3D=1.82e-6)),
    # 782 block partials per camera tensor.  Among 6.3 M list entries some pairs of Gaussians have fp32 depths an ulp apart and
    # stand the other way round in the fp64 run's lists: no seed is free of that.  It is no α/T threshold event — the two orders
    # differ by α₁·α₂·Δc at a pixel, part of the spread measured here, and the kernel sorts by the same fp32 depths as the fp32
    # run — so this case asks for equal radii, ranges and per-tile MEMBERS (`order=False`) and images within FWD_ATOL.
    "large": dict(make=lambda: large_scene(seed=1), with_depth=False, stride=7, order=False,
                  spread=dict(viewmatrix=1.26e-6, projmatrix=2.46e-6, campos=2.46e-6, means3D=1.56e-6)),
}


def pose_bars(name):
    s = POSE_CASES[name]["spread"]
    cam = 10.0 * max(s["viewmatrix"], s["projmatrix"], s["campos"])
    return dict(viewmatrix=cam, projmatrix=cam, campos=cam, means3D=cam)


def pose_gradients(cs, case, seed=0):
    """(dL/dcolor, dL/ddepth or None, tile_filter or None) of a camera-gradient case"""
    from ggrt_official_amd.synthetic import upstream_gradient
    W, H = cs.sc.width, cs.sc.height
    dL = upstream_gradient(W, H, seed=seed)
    dLd = upstream_gradient(W, H, seed=seed + 50)[0] * 0.3 if case["with_depth"] else None
    sel = None
    if case.get("stride"):
        sel, mask = tile_sample(W, H, case["stride"])
        dL = dL * mask
        dLd = None if dLd is None else dLd * mask
    return dL, dLd, sel


# ---- the launch set of tests/test_gpu_camera_family.py: three cameras on one mixed scene ------------------------------------
def launch_set(P=8000, W=182, H=134, D=3, seed=5):
    """(scene, [CameraScene per view]): views that differ in field of view (100°, 60°, 25°), pixel aspect, principal point, pose and background"""
    cs = mixed_scene(P, W, H, D, seed)
    c2w0 = torch.linalg.inv(cs.sc.viewmatrix.double().T)
    step = pose(77, angle=0.2, shift=0.3)
    cs.sc.bg = torch.tensor([0.1, 0.2, 0.3])
    views = [cs]
    for fov, aspect, cx, cy, c2w in ((60.0, 0.85, 0.55, 0.48, c2w0 @ step), (25.0, 1.2, 0.47, 0.56, c2w0 @ torch.linalg.inv(step))):
        view, full, campos, tx, ty = camera(W, H, fov, aspect, cx, cy, c2w)
        views.append(copy_scene(cs, viewmatrix=view, projmatrix=full, campos=campos, tanfovx=tx, tanfovy=ty,
                                bg=torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.5, 0.1]][len(views) - 1])))
    return cs, views


# fp32 against fp64 torch autograd per view of launch_set() (flip-free), rel-L2: viewmatrix, projmatrix, campos
LAUNCH_SET_SPREAD = [(1.43e-5, 5.51e-6, 2.92e-6), (3.78e-7, 3.44e-7, 1.12e-6), (2.86e-6, 2.66e-5, 3.57e-7)]
