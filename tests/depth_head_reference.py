"""The depth head's arithmetic restated in plain torch (any dtype, any device, autograd on): what
`ggrt_official_amd.fused_depth_head` computes with one HIP launch.  Written from the contract (include/ggr_raster.h,
GgrDepthHeadPass); float64 inputs on the CPU make it the reference of tests/test_gpu_depth_head.py, float32 inputs on the device
the torch route the kernels are compared with.

`make_case` draws seeded inputs that obey the index-margin rule, checked at float64: a float32 running sum of <= 64 terms <= 1
errs by about 4e-6, so with every decision 1e-4 away from its boundary the float32 routes must choose the float64 index."""
import torch

FLT_EPSILON = 1.1920928955078125e-07
MARGIN = 1e-4


def split_logits(logits, srf):
    """[C,R,2·s·srf] in the channel order (bucket, surface, {pdf, offset}) → pdf logits, offset logits, each [C,R,srf,s]"""
    n_cam, rays, width = logits.shape
    s = width // (2 * srf)
    l = logits.reshape(n_cam, rays, s, srf, 2).permute(0, 1, 3, 2, 4)
    return l[..., 0], l[..., 1]


def choose_index(pdf, spp, deterministic, u):
    """pdf [..., s] → index [..., spp] (int64)"""
    s = pdf.shape[-1]
    if deterministic:
        return torch.sort(pdf, dim=-1, descending=True, stable=True).indices[..., :spp]    # (stable: ties to the lower bucket)
    npdf = pdf / (FLT_EPSILON + pdf.sum(-1, keepdim=True))
    return torch.searchsorted(npdf.cumsum(-1), u.contiguous(), right=True).clamp(max=s - 1)


def depth_head_reference(logits, xy_raw, ray_xy, near, far, image_shape, num_surfaces, samples_per_ray, deterministic, *,
                         use_transmittance=False, opacity_exponent=1.0, opacity_scale=None, u=None, index=None):
    """→ dict(depths [C,G], opacities [C,G], coordinates [C,G,2], index [C,G]), G = R·srf·spp, sample axis innermost.
    `index` given: taken as it is (the choice is not differentiated either way)."""
    srf, spp = num_surfaces, samples_per_ray
    n_cam, rays, width = logits.shape
    s = width // (2 * srf)
    dt, dev = logits.dtype, logits.device
    pdf_logits, offset_logits = split_logits(logits, srf)
    pdf = torch.softmax(pdf_logits, -1)
    npdf = pdf / (FLT_EPSILON + pdf.sum(-1, keepdim=True))
    if index is None:
        with torch.no_grad():
            index = choose_index(pdf, spp, deterministic, None if u is None else u.reshape(n_cam, rays, srf, spp).to(dt))
    index = index.reshape(n_cam, rays, srf, spp).long()
    rel = (index + torch.sigmoid(offset_logits).gather(-1, index)) / s
    dn = 1 / (near.reshape(-1, 1, 1, 1) + 1e-10)
    df = 1 / (far.reshape(-1, 1, 1, 1) + 1e-10)
    depths = 1 / ((1 - rel) * (dn - df) + df + 1e-10)
    if use_transmittance:
        before = torch.cat([torch.zeros_like(pdf[..., :1]), pdf.cumsum(-1)[..., :-1]], -1)    # Σ_{d<i} pdf_d, a running sum
        q = (pdf / (1 - before + 1e-10)).gather(-1, index)
    else:
        q = npdf.gather(-1, index)
    scale = 1.0 / spp if opacity_scale is None else opacity_scale
    if opacity_exponent == 1.0:
        opacities = scale * q
    else:
        opacities = scale * 0.5 * (1 - (1 - q).clamp(min=0) ** opacity_exponent + q ** (1.0 / opacity_exponent))
    h, w = image_shape
    pixel = torch.tensor([1.0 / w, 1.0 / h], dtype=dt, device=dev)
    xy = ray_xy[None, :, None, :] + (torch.sigmoid(xy_raw.reshape(n_cam, rays, srf, 2)) - 0.5) * pixel
    coordinates = xy[:, :, :, None, :].expand(n_cam, rays, srf, spp, 2)
    g = rays * srf * spp
    return dict(depths=depths.reshape(n_cam, g), opacities=opacities.reshape(n_cam, g), coordinates=coordinates.reshape(n_cam, g, 2),
                index=index.reshape(n_cam, g))


def margin_violations(logits, srf, spp, deterministic, u):
    """bool [C,R,srf]: the rows whose index choice lies within MARGIN of a boundary, at float64"""
    pdf = torch.softmax(split_logits(logits.double(), srf)[0], -1)
    s = pdf.shape[-1]
    if deterministic:
        top = torch.sort(pdf, dim=-1, descending=True).values[..., :min(spp + 1, s)]
        if top.shape[-1] < 2:
            return torch.zeros(pdf.shape[:-1], dtype=torch.bool)
        return ((top[..., :-1] - top[..., 1:]) < MARGIN * top[..., :-1]).any(-1)
    if s < 2:
        return torch.zeros(pdf.shape[:-1], dtype=torch.bool)
    # (the last boundary decides nothing: either side of it clips to s − 1)
    cdf = (pdf / (FLT_EPSILON + pdf.sum(-1, keepdim=True))).cumsum(-1)[..., :-1]
    return ((u.double()[..., :, None] - cdf[..., None, :]).abs() < MARGIN).any(-1).any(-1)


def make_case(n_cam, rays, s, srf, spp, mode, seed=0, use_transmittance=False, opacity_exponent=1.0, image_shape=(16, 24),
              logit_scale=2.0, dtype=torch.float64):
    """Seeded CPU inputs of one depth-head call (mode: "sampled" or "deterministic") that obey the index-margin rule: the rows
    that violate it are redrawn with the next seed, not dropped."""
    deterministic = mode == "deterministic"
    assert mode in ("sampled", "deterministic")

    def draw(sd):
        gen = torch.Generator().manual_seed(sd)
        return (logit_scale * torch.randn(n_cam, rays, 2 * s * srf, generator=gen, dtype=torch.float64),
                torch.rand(n_cam, rays, srf, spp, generator=gen, dtype=torch.float64), gen)

    logits, u, gen = draw(seed)
    xy_raw = torch.randn(n_cam, rays * srf, 2, generator=gen, dtype=torch.float64)
    ray_xy = torch.rand(rays, 2, generator=gen, dtype=torch.float64)
    near = 0.5 + torch.rand(n_cam, generator=gen, dtype=torch.float64)
    far = 20.0 + 80.0 * torch.rand(n_cam, generator=gen, dtype=torch.float64)
    u = u.float().double()     # (the numbers the float32 routes will see)
    logits = logits.float().double()
    for attempt in range(1, 50):
        bad = margin_violations(logits, srf, spp, deterministic, u)
        if not bool(bad.any()):
            break
        l2, u2, _ = draw(seed + attempt)
        if deterministic:
            rows = bad.any(-1)                                         # a ray's surfaces share its row of logits
            logits[rows] = l2.float().double()[rows]
        else:
            u[bad] = u2.float().double()[bad]
    else:
        raise RuntimeError("make_case: the margin rule still fails after 49 redraws")
    case = dict(logits=logits, xy_raw=xy_raw, ray_xy=ray_xy, near=near, far=far, image_shape=image_shape, num_surfaces=srf,
                samples_per_ray=spp, deterministic=deterministic, use_transmittance=use_transmittance,
                opacity_exponent=opacity_exponent, opacity_scale=None, u=None if deterministic else u)
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in case.items()}
