"""Shared helpers of the parity tests: run the CPU oracle / the HIP path on one Scene."""
from __future__ import annotations

import numpy as np
import torch

from ggrt_official_amd.synthetic import Scene
from oracle import c_oracle


# ---- parity bars (BASELINE.json north_star: images "within 1e-4", gradients within 1e-3 rel-L2) -----------------
# The bars below are ONE ORDER above what the HIP path measures against the C oracle on an MI355X (round 2,
# gpurun_out/parity_metrics.jsonl over all -m gpu tests incl. the full-size frames): peak-normalised image PSNR
# 119 … 148 dB (the full-size frames sit at the low end: a handful of threshold flips out of 2 M pixels dominate
# their MSE), ≤ 7e-6 of the pixels off by more than 1e-4, per-tensor gradient rel-L2 5e-7 … 4e-6 — not the
# north-star's loose figures: a regression of an order of magnitude fails.  A threshold flip (α within an ulp of
# 1/255, T·(1-α) of 1e-4) moves one pixel by at most ≈ 4e-3·|c|; everything else must agree to FWD_ATOL.
FWD_ATOL = 1e-4
FLIP_FRACTION = 5e-5
PSNR_MIN = 110.0
GRAD_RTOL = 2e-5


def record_metric(tag: str, **kv):
    """Appends measured parity figures to gpurun_out/parity_metrics.jsonl (scratch; the bars above are set from
    these).  Never fails a test."""
    try:
        import json
        import os
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_metrics.jsonl"), "a") as f:
            f.write(json.dumps(dict(tag=tag, **{k: float(v) for k, v in kv.items()})) + "\n")
    except Exception:
        pass


def check_image(img, ref, name="color", tag="", psnr_min=None, flip_fraction=None, exclude=None):
    """`exclude`: boolean [H, W] mask of pixels that `threshold_flips` has explained — they are left out of every figure."""
    img, ref = np.asarray(img, np.float64), np.asarray(ref, np.float64)
    if exclude is not None:
        img, ref = img[..., ~exclude], ref[..., ~exclude]
    d = np.abs(img - ref)
    peak = max(1.0, float(np.abs(ref).max()))  # depth images are not in [0, 1]: PSNR relative to the peak value
    bad = float((d > FWD_ATOL * peak).mean())
    p = psnr(img, ref) + 20.0 * np.log10(peak)
    record_metric(tag or name, kind=0, psnr=min(p, 999.0), flip_frac=bad, max_abs=float(d.max()))
    # (the fraction is a bar for frames; ONE flipped pixel — its three channels — is within it whatever the image size: a
    #  35 × 151 image has 15 855 values, one of them is already 6.3e-5.  Found by the 240-case soak run of the random sweep.)
    allowed = max(FLIP_FRACTION if flip_fraction is None else flip_fraction, 3.0 / d.size)
    assert bad <= allowed, f"{name}: {bad:.2e} of pixels differ by > {FWD_ATOL * peak}"
    assert d.max() <= 0.02 * peak, f"{name}: max abs diff {d.max()}"
    assert p >= (PSNR_MIN if psnr_min is None else psnr_min), f"{name}: PSNR {p:.1f} dB"


def threshold_flips(st, img, atol=FWD_ATOL):
    """The pixels where `img` differs from the oracle state's image by more than the forward tolerance, each with the list
    entry of its tile that sits nearest to one of the two DISCRETE decisions of the compositing rule — α against 1/255,
    T·(1 − α) against 1e-4 — as (y, x, |d|, Gaussian id, relative distance, the pixel's contributors).  The tile's list is walked in fp32 numpy with the
    oracle's per-Gaussian values.  A distance of a few 1e-7 is an ulp of the exponential: two correct implementations may
    decide differently there and the pixel moves by up to α·T·|c| — a discrete event, not an error.  A 1 500-case soak of the
    random sweep (round 4) left the bars in 10 cases, every one through a pixel within 1e-6 of the α threshold; the statistical bars of
    check_image are sized for frames, a tiny image with one flip exceeds them."""
    d = np.abs(np.asarray(img, np.float64) - st.color.astype(np.float64)).max(0)
    gx = (st.W + 15) // 16
    out = []
    for y, x in zip(*np.nonzero(d > atol)):
        lo, hi = st.ranges[(y // 16) * gx + x // 16]
        T, best, seen = np.float32(1.0), (1e9, -1), []
        for g in st.point_list[lo:hi]:
            dx, dy = np.float32(st.xy[g, 0] - np.float32(x)), np.float32(st.xy[g, 1] - np.float32(y))
            a, b, c, op = (np.float32(v) for v in st.conic_opacity[g])
            power = np.float32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
            if power > 0:
                continue
            alpha = min(np.float32(0.99), op * np.exp(power, dtype=np.float32))
            best = min(best, (abs(float(alpha) * 255.0 - 1.0), int(g)))
            if alpha < np.float32(1.0 / 255.0):
                continue
            test_T = T * (np.float32(1) - alpha)
            best = min(best, (abs(float(test_T) / 1e-4 - 1.0), int(g)))
            if test_T < np.float32(1e-4):
                break
            T = test_T
            seen.append(int(g))
        # (a flip at this pixel moves the transmittance of everything behind the entry by α ≈ 0.4 % and the colour behind
        #  everything in front of it: every contributor of the pixel has one slightly different term in its gradient sums)
        out.append((int(y), int(x), float(d[y, x]), best[1], best[0], seen + [best[1]]))
    return out


GRAD_RTOL_ALL = 1e-3     # the north-star's bar, on the whole tensor, threshold flips included
FLIP_ROWS = 1e-5         # fraction of the Gaussians whose gradient a threshold flip may have touched — strictly
#                          proportional: below 100 k rows NO row is set aside (with a floor of 8 rows a bug
#                          confined to a few Gaussians of a small case was only held to the 1e-3 bar), 10 at 1 M rows


def check_grads(grads, ref, keys, tag="", rtol=None, exclude_rows=None):
    """Per tensor: rel-L2 over ALL rows ≤ 1e-3 (north-star), and rel-L2 ≤ GRAD_RTOL once the few rows with the
    largest error are set aside.  Why rows are set aside: the same α/T threshold flips that move single pixels of the
    image (check_image) add or drop one (pixel, Gaussian) term of a gradient sum — a discrete event, not rounding.
    At C3 (1 M Gaussians, dL/dcolor ≈ 1.6e-7 per pixel) ONE such term in ONE Gaussian is 7.8e-5 of the whole means3D
    gradient norm while every other row agrees to 9e-7 (tests/tools/grad_outliers.py)."""
    for k in keys:
        a = np.asarray(grads[k], np.float64)
        b = np.asarray(ref[k], np.float64)
        rows = a.shape[0] if a.ndim > 1 else a.size
        a2, b2 = a.reshape(rows, -1), b.reshape(rows, -1)
        r_all = rel_l2(a2, b2)
        err = np.linalg.norm(a2 - b2, axis=1)
        drop = min(rows, int(FLIP_ROWS * rows))
        keep = np.ones(rows, bool)
        if exclude_rows is not None and len(exclude_rows):   # (Gaussians at an explained threshold flip: see threshold_flips)
            keep[np.asarray(exclude_rows, np.int64)] = False
            err = np.where(keep, err, 0.0)
            r_all = float(np.linalg.norm((a2 - b2)[keep]) / max(np.linalg.norm(b2[keep]), 1e-30))
        if rows > drop > 0:
            keep[np.argpartition(-err, drop - 1)[:drop]] = False
        r = float(np.linalg.norm((a2 - b2)[keep]) / max(np.linalg.norm(b2[keep]), 1e-30)) if keep.any() else 0.0
        record_metric(f"{tag}:{k}", kind=1, rel_l2=r, rel_l2_all=r_all)
        assert r_all <= GRAD_RTOL_ALL, f"grad {k}: rel-L2 over all rows {r_all:.3e}"
        assert r <= (GRAD_RTOL if rtol is None else rtol), f"grad {k}: rel-L2 {r:.3e} ({drop} rows set aside; all rows {r_all:.3e})"


def oracle_forward(sc: Scene, use_sh=True, use_cov=True, colors=None, sh_cap=3, tight=True, scale_modifier=1.0):
    """``tight=True``: the oracle with the BUILD's tight tile rects — what the product builds by default, so that lists,
    ranges, num_rendered and n_contrib can be compared entry for entry; ``tight=False``: the reference's rects (the
    restatement proper; the product's ``reference_rects=True``).  Images, final_T, radii and gradients are the same in
    both (tests/test_oracle.py::test_tight_rects_change_no_output)."""
    n = lambda t: t.detach().cpu().numpy()
    kw = {}
    if use_sh:
        kw["shs"] = n(sc.shs)
    else:
        kw["colors_precomp"] = n(colors)
    if use_cov:
        kw["cov3D_precomp"] = n(sc.cov3D)
    else:
        kw["scales"] = n(sc.scales)
        kw["rotations"] = n(sc.rotations)
    return c_oracle.forward(n(sc.means3D), n(sc.opacities), n(sc.viewmatrix), n(sc.projmatrix), n(sc.campos),
                            n(sc.bg), sc.width, sc.height, sc.tanfovx, sc.tanfovy, sh_degree=sc.sh_degree,
                            sh_cap=sh_cap, tight_rects=tight, scale_modifier=scale_modifier, **kw)


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def psnr(a, b) -> float:
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def hip_forward_backward(sc: Scene, dL_dcolor: torch.Tensor, use_sh=True, use_cov=True, colors=None,
                         dL_ddepth=None, pose=False, sh_max_degree=3, reference_rects=False, **settings):
    """Runs the product path (GaussianRasterizer on cuda:0).  Returns (color, radii, depth, grads).  `settings`: further
    fields of GaussianRasterizationSettings (scale_modifier, antialiasing, …)."""
    from ggrt_official_amd import GaussianRasterizer
    dev = torch.device("cuda:0")
    s = sc.to(dev)
    leaf = lambda t: t.detach().clone().to(dev).requires_grad_(True)
    means, op = leaf(s.means3D), leaf(s.opacities)
    means2D = torch.zeros_like(means, requires_grad=True)
    kw, leaves = {}, dict(means3D=means, opacities=op, means2D=means2D)
    if use_sh:
        leaves["shs"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = leaf(colors)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = leaf(s.cov3D)
    else:
        leaves["scales"] = kw["scales"] = leaf(s.scales)
        leaves["rotations"] = kw["rotations"] = leaf(s.rotations)
    rs = s.settings()._replace(sh_max_degree=sh_max_degree, reference_rects=reference_rects, **settings)
    if pose:
        view, proj, cam = leaf(s.viewmatrix), leaf(s.projmatrix), leaf(s.campos)
        rs = rs._replace(viewmatrix=view, projmatrix=proj, campos=cam)
        leaves.update(viewmatrix=view, projmatrix=proj, campos=cam)
    color, radii, depth = GaussianRasterizer(rs)(means3D=means, means2D=means2D, opacities=op, **kw)
    loss = (color * dL_dcolor.to(dev)).sum()
    if dL_ddepth is not None:
        loss = loss + (depth * dL_ddepth.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}
    return color.detach().cpu().numpy(), radii.cpu().numpy(), depth.detach().cpu().numpy(), grads


# ---- the depth order of the tile lists, from a forward's own outputs (tests/test_sort_order_reference.py proves these on the
# C oracle; tests/test_gpu_sort_order.py holds every HIP form of the sort to them) ---------------------------------------------
SORT_KEY_BASE = 0x3E4CCCCD   # float32 bits of the near cull, 0.2
SORT_KEY_MAX = 0x3FFFFFFF    # 30 bits: every depth at or beyond 6.8e37 shares this key


def sort_key(depth) -> np.ndarray:
    """The 30-bit depth key of a visible Gaussian (view depth > 0.2): float32 bits less those of 0.2, clamped."""
    bits = np.ascontiguousarray(np.asarray(depth, np.float32)).view(np.uint32).astype(np.int64)
    return np.minimum(bits - SORT_KEY_BASE, SORT_KEY_MAX).astype(np.uint32)


def order_state(state) -> dict:
    """depth [P], radii [P], ranges [T, 2], point_list [N], num_rendered as numpy — of an OracleState or of the dict that
    debug_forward_state returns"""
    get = (lambda k: state[k]) if isinstance(state, dict) else (lambda k: getattr(state, k))
    n = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    out = dict(depth=n(get("depth")).astype(np.float32), radii=n(get("radii")), ranges=n(get("ranges")).astype(np.int64),
               point_list=n(get("point_list")).astype(np.int64))
    out["num_rendered"] = int(get("num_rendered"))
    return out


def assert_lists_in_depth_order(state):
    """Every tile's list is in strictly ascending (depth key, Gaussian id) order: the order of a stable sort by (tile, key)
    over entries emitted in id order.  Strict, because an id occurs once per tile: one comparison covers order and ties."""
    s = order_state(state)
    pl, rg = s["point_list"], s["ranges"]
    assert len(pl) == s["num_rendered"]
    lens = rg[:, 1] - rg[:, 0]
    assert (lens >= 0).all() and int(lens.sum()) == len(pl), "the ranges do not tile the list"
    if len(pl) < 2:
        return
    assert pl.min() >= 0 and pl.max() < len(s["depth"])
    assert (s["radii"][pl] > 0).all(), "a culled Gaussian in a list"
    k64 = (sort_key(s["depth"])[pl].astype(np.uint64) << np.uint64(32)) | pl.astype(np.uint64)
    ok = k64[1:] > k64[:-1]
    starts = rg[lens > 0, 0]
    ok[starts[starts > 0] - 1] = True          # (the first entry of a range has no predecessor in its tile)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        tile = int(np.flatnonzero((rg[:, 0] <= i + 1) & (i + 1 < rg[:, 1]))[0])
        raise AssertionError(f"{int((~ok).sum())} of {len(pl)} list entries are out of (key, id) order; first in tile {tile} at "
                             f"entry {i + 1}: (key {int(k64[i] >> np.uint64(32)):#x}, id {pl[i]}) before "
                             f"(key {int(k64[i + 1] >> np.uint64(32)):#x}, id {pl[i + 1]})")


def assert_same_members(state_a, state_b):
    """Same num_rendered, same ranges, and tile by tile the same SET of ids (whatever their order)."""
    a, b = order_state(state_a), order_state(state_b)
    assert a["num_rendered"] == b["num_rendered"], (a["num_rendered"], b["num_rendered"])
    assert np.array_equal(a["ranges"], b["ranges"]), "tile ranges differ"
    tile = np.repeat(np.arange(len(a["ranges"])), a["ranges"][:, 1] - a["ranges"][:, 0])
    ma = np.sort((tile << 32) | a["point_list"])
    mb = np.sort((tile << 32) | b["point_list"])
    assert np.array_equal(ma, mb), f"{int((ma != mb).sum())} list entries belong to different tiles"
