"""Per-pixel hit lists, torch reference on the lists of the frozen `oracle.torch_raster`.

`pre`, `point_list` and `ranges` come from tests/contributions_reference.py's `lists` (the oracle's `preprocess` + `bin_tiles`,
the opacity compensated when `antialiasing`); `live` and `w` per (entry, pixel) from its `tile_weights` — the oracle's `blend`,
restated.  Per pixel, over its live entries in list order (front to back), with K slots:
    index[k]  = the id of the k-th one        (−1 for k >= count)
    weight[k] = its w                         (0)
    rest      = Σ w of those behind the K-th  (0)
    count     = their number — all of them    (0)
The arithmetic runs in the dtype of `pre` (float32 or float64)."""
import torch

from oracle import torch_raster as tr
from tests import contributions_reference as cr
from tests import picks_reference as pr


def hit_arrays(pre, point_list, ranges, W, H, K):
    """dict of index [K,H,W] (int64), weight [K,H,W], rest [H,W], count [H,W] (int64)"""
    pre = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in pre.items()}
    dt = pre["xy"].dtype
    gx, gy = (W + tr.TILE - 1) // tr.TILE, (H + tr.TILE - 1) // tr.TILE
    index = torch.full((K, H, W), -1, dtype=torch.int64)
    weight = torch.zeros(K, H, W, dtype=dt)
    rest = torch.zeros(H, W, dtype=dt)
    count = torch.zeros(H, W, dtype=torch.int64)
    for tyi in range(gy):
        y0, y1 = tyi * tr.TILE, min(tyi * tr.TILE + tr.TILE, H)
        for txi in range(gx):
            r0, r1 = int(ranges[tyi * gx + txi, 0]), int(ranges[tyi * gx + txi, 1])
            if r1 <= r0:
                continue
            x0, x1 = txi * tr.TILE, min(txi * tr.TILE + tr.TILE, W)
            ids = point_list[r0:r1].to(torch.int64)
            live, w = cr.tile_weights(pre, ids, x0, x1, y0, y1)          # [n, pixels]
            shape = (y1 - y0, x1 - x0)
            rank = torch.cumsum(live.to(torch.int64), 0) - 1                # the slot a live entry would take
            cols = torch.arange(live.shape[1])
            for k in range(K):
                sel = live & (rank == k)                                     # at most one entry per pixel
                has = sel.any(0)
                pos = sel.to(torch.int32).argmax(0)
                index[k, y0:y1, x0:x1] = torch.where(has, ids[pos], torch.full_like(pos, -1)).reshape(shape)
                weight[k, y0:y1, x0:x1] = torch.where(has, w[pos, cols], torch.zeros((), dtype=dt)).reshape(shape)
            behind = live & (rank >= K)
            rest[y0:y1, x0:x1] = torch.where(behind, w, torch.zeros((), dtype=dt)).cumsum(0)[-1].reshape(shape)   # (list order)
            count[y0:y1, x0:x1] = live.sum(0).reshape(shape)
    return dict(index=index, weight=weight, rest=rest, count=count)


def scene_lists(sc, use_sh=True, use_cov=True, colors=None, antialiasing=False, dtype=torch.float32, sh_cap=3):
    """(pre, point_list, ranges) of a `ggrt_official_amd.synthetic.Scene`, computed in `dtype` (as picks_reference.scene_picks)"""
    c = lambda t: t.detach().cpu().to(dtype)
    kw = dict(shs=c(sc.shs)) if use_sh else dict(colors_precomp=c(colors))
    kw.update(dict(cov3D_precomp=c(sc.cov3D)) if use_cov else dict(scales=c(sc.scales), rotations=c(sc.rotations)))
    return cr.lists(c(sc.means3D), c(sc.opacities), c(sc.viewmatrix), c(sc.projmatrix), c(sc.campos), sc.width, sc.height,
                    sc.tanfovx, sc.tanfovy, sc.sh_degree, sh_cap=sh_cap, antialiasing=antialiasing, **kw)


# the reference scenes of tests/test_gpu_hits.py: the pick tests' two (picks_reference.REF_CASES: multi-batch lists and early
# stops; an odd 83×45 frame with partial tiles, scales + rotations, antialiasing) — every pixel of which composites more than
# REF_K entries — and a third of small Gaussians (the covariances scaled by COV_SCALE), where most pixels do not fill their slots:
# P, W, H, D, use_sh, use_cov, antialiasing, seed.  The seeds satisfy the condition check of tests/test_hits_reference.py: the
# float32 and the float64 reference agree on every slot index and every count.
REF_CASES = dict(pr.REF_CASES, C_small_gaussians_unfilled_slots=(1000, 96, 64, 2, True, True, False, 992))
COV_SCALE = {"C_small_gaussians_unfilled_slots": 0.005}
REF_K = 8

_cache = {}


def ref_case(name, dtype=torch.float64, K=REF_K):
    """(scene, colours, hit arrays, pick planes) of a reference scene, the last two from the same lists — computed once per
    process and shared (read only)"""
    from ggrt_official_amd.synthetic import make_scene
    key = (name, dtype, K)
    if key not in _cache:
        P, W, H, D, use_sh, use_cov, aa, seed = REF_CASES[name]
        sc = make_scene(P, W, H, sh_degree=D, seed=seed)
        if name in COV_SCALE:
            sc.cov3D = sc.cov3D * COV_SCALE[name]
        colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
        pre, point_list, ranges = scene_lists(sc, use_sh, use_cov, colors, aa, dtype)
        _cache[key] = (sc, colors, hit_arrays(pre, point_list, ranges, W, H, K), pr.pick_planes(pre, point_list, ranges, W, H))
    return _cache[key]
