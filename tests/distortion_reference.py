"""Depth-distortion torch reference on the lists of the frozen `oracle.torch_raster`, differentiable.

`pre`, `point_list` and `ranges` come from tests/contributions_reference.py's `lists` (the oracle's `preprocess` + `bin_tiles`,
the opacity compensated when `antialiasing`).  The per-(entry, pixel) weights restate the oracle's `blend` line for line —
DIFFERENTIABLY, with its straight-through min(0.99, α) — and the plane is the ordered form

    A_i = Σ_{j<i} w_j      B_i = Σ_{j<i} w_j·d_j      distortion = 2·Σ_i w_i·(d_i·A_i − B_i)

per pixel over its live entries in list order, d the depth value (view z, or `depth_value`), taken relative to the depth value of
the pixel's first live entry (the sum does not depend on the origin; a float32 run's rounding does).  autograd does the backward.
The arithmetic runs in the dtype of `pre` (float32 or float64)."""
import torch

from oracle import torch_raster as tr


def tile_weights(pre, ids, x0, x1, y0, y1):
    """(live [n, pixels] bool, w [n, pixels], differentiable) of one tile's list `ids` over its pixels — the oracle's `blend`"""
    dt = pre["xy"].dtype
    ys, xs = torch.meshgrid(torch.arange(y0, y1, dtype=dt), torch.arange(x0, x1, dtype=dt), indexing="ij")
    pixx, pixy = xs.reshape(-1), ys.reshape(-1)
    xy, con, op = pre["xy"][ids], pre["conic"][ids], pre["opacity"][ids]
    dx = xy[:, 0:1] - pixx[None]
    dy = xy[:, 1:2] - pixy[None]
    power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
    araw = op[:, None] * torch.exp(power)
    alpha = araw + (araw.clamp(max=tr.ALPHA_MAX) - araw).detach()
    valid = (power <= 0) & (alpha >= tr.ALPHA_MIN)
    aeff = torch.where(valid, alpha, torch.zeros_like(alpha))
    Tafter = torch.cumprod(1.0 - aeff, 0)
    Tbefore = torch.cat([torch.ones_like(Tafter[:1]), Tafter[:-1]], 0)
    with torch.no_grad():
        stop = (Tafter < tr.T_MIN) & valid
        live = valid & ~(torch.cumsum(stop.to(torch.int32), 0) > 0)
    return live, torch.where(live, aeff * Tbefore, torch.zeros_like(aeff))


def _tiles(ranges, W, H):
    gx, gy = (W + tr.TILE - 1) // tr.TILE, (H + tr.TILE - 1) // tr.TILE
    for tyi in range(gy):
        for txi in range(gx):
            r0, r1 = int(ranges[tyi * gx + txi, 0]), int(ranges[tyi * gx + txi, 1])
            if r1 > r0:
                yield r0, r1, txi * tr.TILE, min(txi * tr.TILE + tr.TILE, W), tyi * tr.TILE, min(tyi * tr.TILE + tr.TILE, H)


def distortion_plane(pre, point_list, ranges, W, H, depth_value=None, brute_force=False):
    """[H,W], differentiable in everything `pre` (and `depth_value` [P], default `pre["depth"]`) is.  `brute_force`: the
    unordered Σ_{i,j} w_i·w_j·|d_i − d_j| instead (equal whenever d does not decrease along the lists)."""
    dt = pre["xy"].dtype
    dval = (pre["depth"] if depth_value is None else depth_value).to(dt)
    idx, vals = [], []
    for r0, r1, x0, x1, y0, y1 in _tiles(ranges, W, H):
        ids = point_list[r0:r1].to(torch.int64)
        live, w = tile_weights(pre, ids, x0, x1, y0, y1)                 # [n, pixels]
        d = dval[ids]
        if brute_force:
            q = (w * ((d[:, None] - d[None, :]).abs() @ w)).sum(0)
        else:
            first = live.to(torch.int32).argmax(0)                       # (no live entry: every w is 0)
            dr = d[:, None] - d[first][None].detach()
            wd = w * dr
            A = torch.cumsum(w, 0) - w
            B = torch.cumsum(wd, 0) - wd
            q = 2.0 * (w * (dr * A - B)).sum(0)
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        idx.append((ys * W + xs).reshape(-1))
        vals.append(q)
    flat = torch.zeros(H * W, dtype=dt)
    if idx:
        flat = flat.index_add(0, torch.cat(idx), torch.cat(vals))        # (out of place: differentiable; a pixel occurs once)
    return flat.reshape(H, W)


def rasterize_distortion(means3D, opacities, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, sh_degree=0, aux=None,
                         features=None, **kw):
    """dict of the oracle's planes over ONE preprocess + list build, all differentiable: color [3,H,W], depth [H,W] (Σ d·w),
    alpha [H,W], features [K,H,W] (when given), distortion [H,W]; + radii, and `longest` / `stopped` / `covered` of
    tests/picks_reference.py (the longest tile list, the pixels that stop before their list ends, the pixels with an entry).
    `aux` [P]: the depth value in place of view z.  `kw` as contributions_reference.lists (shs | colors_precomp, cov3D_precomp |
    scales + rotations, sh_cap, antialiasing)."""
    from tests import picks_reference as pr
    aa = kw.pop("antialiasing", False)
    pre = tr.preprocess(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree, depth_grad=True, **kw)
    if aa:
        from tests.aa_reference import aa_scale
        pre = dict(pre)
        pre["opacity"] = pre["opacity"] * aa_scale(pre["conic"])
    point_list, ranges, _keys, _n = tr.bin_tiles(pre, W, H)
    dt = pre["xy"].dtype
    color, _t, _n, depth = tr.blend(pre, point_list, ranges, bg, W, H, aux=aux)
    one, zero = torch.ones(3, dtype=dt), torch.zeros(3, dtype=dt)
    alpha = 1.0 - (tr.blend(pre, point_list, ranges, one, W, H, want_depth=False)[0][0] -
                   tr.blend(pre, point_list, ranges, zero, W, H, want_depth=False)[0][0])
    out = dict(color=color, depth=depth, alpha=alpha, radii=pre["radii"].to(torch.int32),
               distortion=distortion_plane(pre, point_list, ranges, W, H, depth_value=aux))
    if features is not None:
        planes = []
        for k0 in range(0, features.shape[1], 3):
            sl = features[:, k0:k0 + 3].to(dt)
            n = sl.shape[1]
            p2 = dict(pre)
            p2["rgb"] = torch.cat([sl, torch.zeros(sl.shape[0], 3 - n, dtype=dt)], dim=1)
            planes.append(tr.blend(p2, point_list, ranges, zero, W, H, want_depth=False)[0][:n])
        out["features"] = torch.cat(planes, dim=0)
    picks = pr.pick_planes(pre, point_list, ranges, W, H)
    out.update(longest=picks["longest"], stopped=picks["stopped"], covered=int((picks["count"] > 0).sum()))
    return out


# ---- the scene of tests/test_gpu_distortion.py -----------------------------------------------------------------------------------
GPU_W, GPU_H, GPU_P = 40, 24, 700   # 3 × 2 tiles, ragged right and bottom


def clustered_scene(seed=1301, P=GPU_P, W=GPU_W, H=GPU_H, sh_degree=1, squeeze=0.45, opacity=1.0):
    """A `make_scene` frame whose Gaussians are pulled towards the centre of tile (1, 0), so that this tile's list holds more
    than two staging batches (512 entries), with opacities left high enough that the pixels there stop early while pixels near
    the frame's ragged edges run to the end of their lists."""
    from ggrt_official_amd.synthetic import make_scene
    sc = make_scene(P, W, H, sh_degree=sh_degree, seed=seed)
    fpx = W / (2.0 * sc.tanfovx)
    m = sc.means3D.double()
    u, v, z = m[:, 0] / m[:, 2] * fpx + 0.5 * W, m[:, 1] / m[:, 2] * fpx + 0.5 * H, m[:, 2]
    u, v = 24.0 + squeeze * (u - 24.0), 8.0 + squeeze * (v - 8.0)
    sc.means3D = torch.stack([(u - 0.5 * W) / fpx * z, (v - 0.5 * H) / fpx * z, z], -1).float()
    sc.opacities = (sc.opacities * opacity).clamp(max=1.0)
    return sc


def scene_inputs(sc, dtype, use_sh=True, use_cov=True, colors=None, leaf=False):
    """the keyword inputs of `rasterize_distortion` for a Scene, in `dtype`; `leaf`: every tensor a fresh leaf that requires grad"""
    c = (lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)) if leaf else (lambda t: t.detach().cpu().to(dtype))
    kw = dict(means3D=c(sc.means3D), opacities=c(sc.opacities), viewmatrix=c(sc.viewmatrix), projmatrix=c(sc.projmatrix),
              campos=c(sc.campos))
    kw.update(dict(shs=c(sc.shs)) if use_sh else dict(colors_precomp=c(colors)))
    kw.update(dict(cov3D_precomp=c(sc.cov3D)) if use_cov else dict(scales=c(sc.scales), rotations=c(sc.rotations)))
    return kw


def run_reference(sc, kw, aux=None, features=None, antialiasing=False):
    return rasterize_distortion(bg=sc.bg.to(kw["means3D"].dtype), W=sc.width, H=sc.height, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy,
                                sh_degree=sc.sh_degree, sh_cap=3, aux=aux, features=features, antialiasing=antialiasing, **kw)
