"""Differentiable per-pixel hit lists, torch reference on the lists of the frozen `oracle.torch_raster`.

tests/hits_reference.py's `hit_arrays` WITHOUT the detach: `pre`, `point_list` and `ranges` come from the oracle's `preprocess` +
`bin_tiles` (the opacity compensated when `antialiasing`), the per-(entry, pixel) weights from tests/distortion_reference.py's
`tile_weights` — the oracle's `blend` restated DIFFERENTIABLY, with its straight-through min(0.99, α) and with the skip, threshold
and stop decisions as constants.  Per pixel, over its live entries in list order, with K slots:
    index[k]  = the id of the k-th one        (−1 for k >= count)       not differentiable
    weight[k] = its w                         (0)                        differentiable
    rest      = Σ w of those behind the K-th  (0)                        differentiable
    count     = their number — all of them    (0)                        not differentiable
autograd does the backward.  The arithmetic runs in the dtype of `pre` (float32 or float64).

`closed_form_dalpha` is the formula the kernel implements (include/ggr_raster.h GgrHitGradPass), for the self-checks."""
import torch

from oracle import torch_raster as tr
from tests import distortion_reference as dr
from tests import hits_reference as hr


def tile_slots(live, w, ids, K):
    """One tile: (index [K, pixels] int64, weight [K, pixels], rest [pixels], count [pixels] int64) from `tile_weights`' result"""
    dt = w.dtype
    npix = live.shape[1]
    rank = torch.cumsum(live.to(torch.int64), 0) - 1                     # the slot a live entry would take
    e, p = torch.nonzero(live & (rank < K), as_tuple=True)               # (a (slot, pixel) pair occurs at most once)
    k = rank[e, p]
    index = torch.full((K, npix), -1, dtype=torch.int64).index_put((k, p), ids[e])
    weight = torch.zeros(K, npix, dtype=dt).index_put((k, p), w[e, p])   # (out of place: differentiable)
    rest = torch.where(live & (rank >= K), w, torch.zeros((), dtype=dt)).sum(0)
    return index, weight, rest, live.sum(0)


def hit_arrays(pre, point_list, ranges, W, H, K, tiles=None):
    """dict of index [K,H,W] (int64), weight [K,H,W], rest [H,W], count [H,W] (int64); weight and rest differentiable in
    everything `pre` is.  `tiles`: the cached result of `tile_graph` over the same arguments (else computed here)."""
    dt = pre["xy"].dtype
    tiles = tile_graph(pre, point_list, ranges, W, H) if tiles is None else tiles
    pix, idx, wgt, rst, cnt = [], [], [], [], []
    for flat, ids, live, w in tiles:
        i, wk, r, c = tile_slots(live, w, ids, K)
        pix.append(flat); idx.append(i); wgt.append(wk); rst.append(r); cnt.append(c)
    index = torch.full((K, H * W), -1, dtype=torch.int64)
    weight, rest = torch.zeros(K, H * W, dtype=dt), torch.zeros(H * W, dtype=dt)
    count = torch.zeros(H * W, dtype=torch.int64)
    if pix:
        at = torch.cat(pix)                                              # (a pixel occurs once)
        index[:, at] = torch.cat(idx, 1)
        count[at] = torch.cat(cnt)
        weight = weight.index_add(1, at, torch.cat(wgt, 1))              # (out of place: differentiable)
        rest = rest.index_add(0, at, torch.cat(rst))
    return dict(index=index.reshape(K, H, W), weight=weight.reshape(K, H, W), rest=rest.reshape(H, W), count=count.reshape(H, W))


def tile_graph(pre, point_list, ranges, W, H):
    """Per non-empty tile: (flat pixel indices, list ids, live, w) — the part of `hit_arrays` that does not depend on K, so that
    several K (and several losses) share one forward graph"""
    out = []
    for r0, r1, x0, x1, y0, y1 in dr._tiles(ranges, W, H):
        ids = point_list[r0:r1].to(torch.int64)
        live, w = dr.tile_weights(pre, ids, x0, x1, y0, y1)
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        out.append(((ys * W + xs).reshape(-1), ids, live, w))
    return out


def preprocess_lists(kw, sc, antialiasing=False):
    """(pre, point_list, ranges) of a Scene from the keyword inputs of `distortion_reference.scene_inputs` (differentiable when
    those are leaves)"""
    pre = tr.preprocess(W=sc.width, H=sc.height, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, sh_degree=sc.sh_degree, sh_cap=3,
                        depth_grad=True, **kw)
    if antialiasing:
        from tests.aa_reference import aa_scale
        pre = dict(pre)
        pre["opacity"] = pre["opacity"] * aa_scale(pre["conic"])
    point_list, ranges, _keys, _n = tr.bin_tiles(pre, sc.width, sc.height)
    return pre, point_list, ranges


def closed_form_dalpha(alpha, g):
    """dL/dα_i of one pixel whose live entries have the opacities-at-the-pixel `alpha` [n] and the upstream gradients `g` [n]
    (g_i = dL_dweight[i] for i < K, dL_drest behind): T_i·g_i − S_i/(1−α_i), S_i = total − Σ_{j<=i} g_j·w_j"""
    T = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(1.0 - alpha, 0)[:-1]])
    w = alpha * T
    total = (g * w).sum()
    S = total - torch.cumsum(g * w, 0)
    return T * g - S / (1.0 - alpha)


# ---- the scenes of tests/test_gpu_hits_grad.py: hits_reference.REF_CASES, unchanged.  tests/test_hits_grad_reference.py checks that
# on every one of them the float32 and the float64 reference agree on every slot index and every count at K = 1, 8 and 32.
REF_CASES = hr.REF_CASES
COV_SCALE = hr.COV_SCALE
REF_KS = (1, 8, 32)

_cache = {}


def ref_scene(name):
    """(scene, colours) of a reference scene, as hits_reference.ref_case builds them"""
    from ggrt_official_amd.synthetic import make_scene
    if ("scene", name) not in _cache:
        P, W, H, D, _use_sh, _use_cov, _aa, seed = REF_CASES[name]
        sc = make_scene(P, W, H, sh_degree=D, seed=seed)
        if name in COV_SCALE:
            sc.cov3D = sc.cov3D * COV_SCALE[name]
        _cache[("scene", name)] = (sc, torch.rand(P, 3, generator=torch.Generator().manual_seed(seed)))
    return _cache[("scene", name)]


def ref_graph(name, dtype=torch.float64, antialiasing=None):
    """(leaves by name, pre, point_list, ranges, tiles) of a reference scene with every input a leaf that requires grad —
    computed once per process and shared: `ref_hits` differentiates this one graph for every K and every loss"""
    key = ("graph", name, dtype, antialiasing)
    if key not in _cache:
        sc, colors = ref_scene(name)
        _P, W, H, _D, use_sh, use_cov, aa, _seed = REF_CASES[name]
        aa = aa if antialiasing is None else antialiasing
        kw = dr.scene_inputs(sc, dtype, use_sh, use_cov, colors, leaf=True)
        pre, point_list, ranges = preprocess_lists(kw, sc, aa)
        _cache[key] = (kw, pre, point_list, ranges, tile_graph(pre, point_list, ranges, W, H))
    return _cache[key]


def ref_hits(name, K, dtype=torch.float64, antialiasing=None):
    """(leaves, hit arrays) of a reference scene at K slots, on the shared graph (read only; differentiate it with
    `torch.autograd.grad(..., retain_graph=True)`)"""
    key = ("hits", name, K, dtype, antialiasing)
    if key not in _cache:
        kw, pre, point_list, ranges, tiles = ref_graph(name, dtype, antialiasing)
        _P, W, H = REF_CASES[name][:3]
        _cache[key] = (kw, hit_arrays(pre, point_list, ranges, W, H, K, tiles))
    return _cache[key]


def ref_grads(name, K, G, Gr, dtype=torch.float64, antialiasing=None):
    """gradients (numpy, by input name) of Σ G·weight + Σ Gr·rest on a reference scene; None for G / Gr = no such term"""
    kw, arr = ref_hits(name, K, dtype, antialiasing)
    loss = 0.0
    if G is not None:
        loss = loss + (arr["weight"] * G.to(dtype)).sum()
    if Gr is not None:
        loss = loss + (arr["rest"] * Gr.to(dtype)).sum()
    names = list(kw)
    got = torch.autograd.grad(loss, [kw[k] for k in names], retain_graph=True, allow_unused=True)
    return {k: (torch.zeros_like(kw[k]) if g is None else g).numpy() for k, g in zip(names, got)}
