"""Per-Gaussian absolute screen-space positional gradients (absgrad), torch reference on the lists of the frozen
`oracle.torch_raster`.

`pre`, `point_list` and `ranges` come from tests/contributions_reference.py's `lists` (the oracle's `preprocess` + `bin_tiles`,
the opacity compensated when `antialiasing`).  Per tile the oracle's `blend` is restated line for line from an [n, pixels] alpha
tensor that is a LEAF: the tile's pixels of the planes a forward blends,

    C = Σ w_i c_i + T_f·bg      D = Σ w_i d_i      A = 1 − T_f          (w = α·T, d the depth value: view z or `depth_value`)

are functions of it, and autograd of Σ_p (g_C·C + g_D·D + g_A·A) gives ∂L_p/∂α_{i,p} per ELEMENT — exact, because column p of
the alpha tensor feeds pixel p only.  The analytic ∂α/∂mean2D (straight through the 0.99 clamp, NDC-scaled as dL_dmeans2D is)

    gx_{i,p} = ½W·∂L_p/∂α_{i,p}·o_i·G_{i,p}·(−(cxx·dx + cxy·dy))      gy_{i,p} = ½H·∂L_p/∂α_{i,p}·o_i·G_{i,p}·(−(cyy·dy + cxy·dx))

with (dx, dy) = mean2D_i − p is applied per element; absgrad = Σ_p |g|, signed = Σ_p g.  The planes are returned too
(tests/test_absgrad_reference.py holds them against `tr.blend`'s).  The arithmetic runs in the dtype of `pre` (float32 or
float64)."""
import torch

from oracle import torch_raster as tr
from tests import contributions_reference as cr
from tests import distortion_reference as dr


def absgrad_from_lists(pre, point_list, ranges, bg, W, H, gC, gD=None, gA=None, depth_value=None):
    """(absgrad [P,2], signed [P,2], planes) of one view.  gC [3,H,W]; gD, gA [H,W] or None (= zero); `depth_value` [P] in place of
    `pre["depth"]`.  planes: dict(color [3,H,W], depth [H,W], alpha [H,W]) as blended from the alpha leaves."""
    pre = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in pre.items()}
    dt = pre["xy"].dtype
    P = pre["xy"].shape[0]
    bg = bg.detach().to(dt)
    gC = gC.detach().to(dt)
    gD = torch.zeros(H, W, dtype=dt) if gD is None else gD.detach().to(dt)
    gA = torch.zeros(H, W, dtype=dt) if gA is None else gA.detach().to(dt)
    dval = (pre["depth"] if depth_value is None else depth_value.detach()).to(dt)
    absg, signed = torch.zeros(P, 2, dtype=dt), torch.zeros(P, 2, dtype=dt)
    color = bg[:, None, None].expand(3, H, W).clone()
    depth, alpha_img = torch.zeros(H, W, dtype=dt), torch.zeros(H, W, dtype=dt)
    for r0, r1, x0, x1, y0, y1 in dr._tiles(ranges, W, H):
        ids = point_list[r0:r1].to(torch.int64)
        ys, xs = torch.meshgrid(torch.arange(y0, y1, dtype=dt), torch.arange(x0, x1, dtype=dt), indexing="ij")
        pixx, pixy = xs.reshape(-1), ys.reshape(-1)
        xy, con, op = pre["xy"][ids], pre["conic"][ids], pre["opacity"][ids]
        dx = xy[:, 0:1] - pixx[None]
        dy = xy[:, 1:2] - pixy[None]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        G = torch.exp(power)
        araw = op[:, None] * G
        alpha = araw.clamp(max=tr.ALPHA_MAX).clone().requires_grad_(True)      # the leaf: [n, pixels]
        valid = (power <= 0) & (alpha >= tr.ALPHA_MIN)
        aeff = torch.where(valid, alpha, torch.zeros_like(alpha))
        one_m = 1.0 - aeff
        Tafter = torch.cumprod(one_m, 0)
        Tbefore = torch.cat([torch.ones_like(Tafter[:1]), Tafter[:-1]], 0)
        with torch.no_grad():
            stop = (Tafter < tr.T_MIN) & valid
            live = valid & ~(torch.cumsum(stop.to(torch.int32), 0) > 0)
        w = torch.where(live, aeff * Tbefore, torch.zeros_like(aeff))
        Tfin = torch.prod(torch.where(live, one_m, torch.ones_like(one_m)), 0)
        c = (w[:, :, None] * pre["rgb"][ids][:, None, :]).sum(0) + Tfin[:, None] * bg[None]      # [pixels, 3]
        dz = (w * dval[ids][:, None]).sum(0)
        acc = 1.0 - Tfin
        h, w_ = y1 - y0, x1 - x0
        gc = gC[:, y0:y1, x0:x1].reshape(3, -1).T
        loss = (c * gc).sum() + (dz * gD[y0:y1, x0:x1].reshape(-1)).sum() + (acc * gA[y0:y1, x0:x1].reshape(-1)).sum()
        (dL_dalpha,) = torch.autograd.grad(loss, alpha)
        zero = torch.zeros_like(araw)
        # (masked: where power > 0 the unclamped o·G may overflow; such an entry is not live and its ∂L/∂α is 0)
        gx = torch.where(live, 0.5 * W * dL_dalpha * araw * (-(con[:, 0:1] * dx + con[:, 1:2] * dy)), zero)
        gy = torch.where(live, 0.5 * H * dL_dalpha * araw * (-(con[:, 2:3] * dy + con[:, 1:2] * dx)), zero)
        absg.index_add_(0, ids, torch.stack([gx.abs().sum(1), gy.abs().sum(1)], -1))            # (an id occurs once per tile)
        signed.index_add_(0, ids, torch.stack([gx.sum(1), gy.sum(1)], -1))
        color[:, y0:y1, x0:x1] = c.detach().T.reshape(3, h, w_)
        depth[y0:y1, x0:x1] = dz.detach().reshape(h, w_)
        alpha_img[y0:y1, x0:x1] = acc.detach().reshape(h, w_)
    return absg, signed, dict(color=color, depth=depth, alpha=alpha_img)


def affine_depth_value(pre, a, b):
    """the depth value of `aux_affine=(a, b)` at input scale 1: max(a + b·z, 0)"""
    return (a + b * pre["depth"].detach()).clamp(min=0.0)


def scene_absgrad(sc, dtype, gC, gD=None, gA=None, use_sh=True, use_cov=True, colors=None, aux=None, aux_affine=None,
                  antialiasing=False, view=None):
    """`absgrad_from_lists` of a `ggrt_official_amd.synthetic.Scene` in `dtype` → (absgrad, signed, planes, pixel_count [P]).
    `aux` [P]: the depth value (aux_precomp); `aux_affine` (a, b); `view`: (viewmatrix, projmatrix, campos, bg) in place of the
    scene's own camera."""
    c = lambda t: t.detach().cpu().to(dtype)
    kw = dict(shs=c(sc.shs)) if use_sh else dict(colors_precomp=c(colors))
    kw.update(dict(cov3D_precomp=c(sc.cov3D)) if use_cov else dict(scales=c(sc.scales), rotations=c(sc.rotations)))
    vm, pm, cam, bg = (sc.viewmatrix, sc.projmatrix, sc.campos, sc.bg) if view is None else view
    pre, point_list, ranges = cr.lists(c(sc.means3D), c(sc.opacities), c(vm), c(pm), c(cam), sc.width, sc.height, sc.tanfovx,
                                       sc.tanfovy, sc.sh_degree, sh_cap=3, antialiasing=antialiasing, **kw)
    dval = None
    if aux is not None:
        dval = c(aux)
    elif aux_affine is not None:
        dval = affine_depth_value(pre, *aux_affine)
    absg, signed, planes = absgrad_from_lists(pre, point_list, ranges, c(bg), sc.width, sc.height, gC, gD, gA, depth_value=dval)
    count = cr.reduce_lists(pre, point_list, ranges, sc.width, sc.height)[2]
    return absg, signed, planes, count


def launch_set_absgrad(scenes, views, dtype, gC, gD=None, gA=None, **kw):
    """The launch-set wrapper: V views, `scenes[v]` the Gaussian set view v renders and `views[v]` its (viewmatrix, projmatrix,
    campos, bg); gC [V,3,H,W], gD / gA [V,H,W] or None → (absgrad [V,P,2], signed [V,P,2])."""
    outs = [scene_absgrad(scenes[v], dtype, gC[v], None if gD is None else gD[v], None if gA is None else gA[v], view=views[v],
                          **kw)[:2] for v in range(len(views))]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


# ---- the scene and the upstream gradients of tests/test_gpu_absgrad.py ---------------------------------------------------------
GPU_W, GPU_H, GPU_P = dr.GPU_W, dr.GPU_H, dr.GPU_P
GPU_SEED = 1301   # `clustered_scene`'s default: tests/test_absgrad_reference.py asserts the cancellation condition on it
GPU_BG = (0.3, 0.6, 0.1)


def gpu_scene(seed=GPU_SEED):
    """`distortion_reference.clustered_scene` with a NON-ZERO background, so that the T_f·u_bg term is live"""
    sc = dr.clustered_scene(seed=seed)
    sc.bg = torch.tensor(GPU_BG)
    return sc


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def upstream(seed=1400, W=GPU_W, H=GPU_H):
    """dict(gC [3,H,W], gD [H,W], gA [H,W]): the upstream gradients of the colour, depth and alpha planes; the four left-most
    columns of all three exactly zero (those pixels take no entry in the pass)"""
    from ggrt_official_amd.synthetic import upstream_gradient
    g = dict(gC=upstream_gradient(W, H, seed=seed), gD=_rand(H, W, seed=seed + 1) / (10.0 * H * W),
             gA=_rand(H, W, seed=seed + 2) / (H * W))
    for v in g.values():
        v[..., :4] = 0.0
    return g


def colors(P=GPU_P, seed=1340):
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))


def aux_value(sc):
    """a depth value that is not view z"""
    return (sc.means3D[:, 2] * 0.5 + 1.0).sqrt().contiguous()


AFFINE = (0.25, 0.5)

# the four input forms of the GPU comparison: the keywords of `scene_absgrad`, and which gradients the loss has
FORMS = {
    "a_sh_cov_colour_only": dict(use_sh=True, use_cov=True, depth=False, alpha=False),
    "b_colours_scale_rot_aux_depth_alpha": dict(use_sh=False, use_cov=False, aux=True, depth=True, alpha=True),
    "c_form_b_antialiased": dict(use_sh=False, use_cov=False, aux=True, depth=True, alpha=True, antialiasing=True),
    "d_aux_affine_depth": dict(use_sh=True, use_cov=True, affine=True, depth=True, alpha=False),
}


def form_reference(form, dtype=torch.float64, sc=None, g=None):
    """(absgrad, signed, planes, pixel_count) of one of FORMS on the GPU scene under `upstream()`"""
    f = FORMS[form]
    sc = gpu_scene() if sc is None else sc
    g = upstream() if g is None else g
    return scene_absgrad(sc, dtype, g["gC"], g["gD"] if f["depth"] else None, g["gA"] if f["alpha"] else None,
                         use_sh=f["use_sh"], use_cov=f["use_cov"], colors=colors(), aux=aux_value(sc) if f.get("aux") else None,
                         aux_affine=AFFINE if f.get("affine") else None, antialiasing=f.get("antialiasing", False))
