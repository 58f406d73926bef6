"""Every form of the depth sort — per-tile LDS sort, global bucket form, global three radix passes — against an INDEPENDENT
order reference on adversarial keys (`-m gpu`).  The reference is numpy (tests/helpers.py): every tile's list must be in strictly
ascending (depth key, Gaussian id) order, with the members of the three-pass form's lists; the scenes (tests/sort_scenes.py) each
assert the property that makes them adversarial on the HIP path's own depths and radii, and a numpy model of the sort routine's
branches says which route every list takes — held to the per-tile sort's slow-route counter.  Sorting is exact: no tolerance.

  1. two depth planes one ulp apart, interleaved with a period that divides 256, in ONE bucket of more than 8192 keys: the
     bucket form must notice that the bucket is not constant (every thread of the copying workgroup sees one key only), fall
     back to three passes inside the call and remember;
  2. bit-pattern keys for route 1 / route 2 of tile_sort_body, 1 … 4 passes, digits of <= 6 and > 6 bits, every register class;
     the same patterns as a whole frame's depth distribution for the bucket form's range variant;
  3. depths at and beyond the last key (6.8e37 … 3e38, +inf);
  4. a launch set of four views of which one meets case 1."""
import numpy as np
import pytest
import torch

from ggrt_official_amd.synthetic import camera_matrices, make_scene
from tests import sort_scenes as S
from tests.helpers import assert_lists_in_depth_order, assert_same_members, oracle_forward

pytestmark = pytest.mark.gpu
IMAGES = ("color", "out_depth", "radii", "final_T", "n_contrib")


def _state(sc, mode, **kw):
    from ggrt_official_amd.rasterizer import debug_forward_state, last_forward_sort_form
    s = sc.to("cuda:0")
    out = debug_forward_state(s.means3D, s.opacities, s.settings()._replace(depth_sort=mode, **kw), shs=s.shs,
                              cov3D_precomp=s.cov3D)
    return out, last_forward_sort_form()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    from ggrt_official_amd.rasterizer import clear_list_hints
    monkeypatch.delenv("GGR_GLOBAL_SORT", raising=False)
    monkeypatch.delenv("GGR_DEPTH_SORT", raising=False)
    clear_list_hints()
    yield
    clear_list_hints()


def _check_forms(sc, modes=("global", "per_tile"), oracle=True, sync_free=False):
    """Every form, in the exact mode (first call of a shape) and with guessed buffers (second call): lists in depth order, the
    three-pass form's members, bit-equal images; the oracle's lists entry for entry.  Returns {mode: [form of call 1, of call 2]}
    and the three-pass state."""
    from ggrt_official_amd.rasterizer import clear_list_hints
    three, how = _state(sc, "global_3pass")
    assert how == "3pass"
    assert_lists_in_depth_order(three)
    forms = {}
    for mode in modes:
        clear_list_hints()
        forms[mode] = []
        for call in range(2):
            out, how = _state(sc, mode)
            forms[mode].append(how)
            assert_lists_in_depth_order(out)
            assert_same_members(out, three)
            for k in IMAGES:
                assert torch.equal(out[k], three[k]), (mode, call, how, k)
        if sync_free:          # the caller's buffer, no read-back: nothing to fall back with (the global sort runs three passes)
            out, how = _state(sc, mode, list_capacity=int(1.25 * three["num_rendered"]) + 4096)
            for k in IMAGES + ("ranges",):
                assert torch.equal(out[k], three[k]), (mode, "sync-free", how, k)
    if oracle:
        st = oracle_forward(sc)
        assert np.array_equal(three["ranges"].cpu().numpy(), st.ranges)
        assert np.array_equal(three["point_list"].cpu().numpy().astype(np.uint32), st.point_list)
    return forms, three


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def _planes(period, gap):
    base, _ = _state(S.interleaved_planes_scene(period), "global_3pass")
    vis = base["radii"].cpu().numpy() > 0
    return S.interleaved_planes_scene(period, gap, visible=vis), vis


@pytest.mark.parametrize("period,gap", [(2, 1), (4, 1), (64, 1), (256, 1), (3, 1), (2, 100)])
def test_interleaved_planes_in_one_oversized_bucket(period, gap):
    """Periods 2 … 256: every thread of the workgroup that copies the oversized bucket sees ONE key; period 3 is the control
    (threads see both).  Either way the bucket is not constant: the call falls back to three passes, and the host remembers."""
    sc, vis = _planes(period, gap)
    forms, three = _check_forms(sc, sync_free=True)
    S.check_interleaved(three, period, vis)
    print(f"period {period} gap {gap}: forms {forms}")
    assert forms["global"] == ["fell_back", "3pass"], forms
    assert forms["per_tile"] == ["per_tile", "per_tile"], forms


def test_single_plane_is_still_copied_without_a_fault():
    sc = S.interleaved_planes_scene(2)          # (no visibility given: everything on one plane)
    forms, three = _check_forms(sc)
    assert forms["global"] == ["buckets", "buckets"], forms
    (n, distinct), = S.bucket_routes(three)[1]      # one oversized bucket, of one key
    assert n > S.CAP_LARGE and distinct == 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def _slow_route_counter(sc):
    """word 3 of ggr_sort_stats_async after one per-tile forward: the list entries of the tiles that took route 2"""
    from ggrt_official_amd import _lib
    from tests.test_gpu_tile_sort import debug_state_geom
    st = debug_state_geom(sc)
    words = torch.zeros(4, dtype=torch.int32).pin_memory()
    assert _lib.load().ggr_sort_stats_async(st["geom"].data_ptr(), sc.means3D.shape[0], words.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return int(words[3])


def _one_tile(sc, K, route, nbits=None, npass=None):
    from ggrt_official_amd.rasterizer import clear_list_hints
    forms, three = _check_forms(sc, sync_free=K in (300, 5000))
    m = S.check_one_tile(three, K, route, nbits=nbits, npass=npass)
    assert forms["per_tile"] == ["per_tile", "per_tile"], forms
    routes, slow = S.tile_routes(three)
    clear_list_hints()
    counted = _slow_route_counter(sc)
    print(f"route {route} nbits {m['nbits']} K {K}: tile passes {m['npass']} digit {m['digit']}; slow-route entries model {slow} "
          f"counter {counted}; global {forms['global']}, buckets reach {sorted(S.bucket_routes(three)[0])}")
    assert counted == slow, (counted, slow)
    assert (slow >= K) == (route == 2)


@pytest.mark.parametrize("route,nbits,K", S.one_tile_cases())
def test_bit_patterns_through_every_route_and_class(route, nbits, K):
    _one_tile(S.one_tile_scene(S.pattern_depths(S.key_pattern(route, nbits, K, seed=K)), seed=K), K, route, nbits=nbits)


@pytest.mark.parametrize("K", [300, 3000, 8192])
def test_four_passes_per_tile(K):
    _one_tile(S.one_tile_scene(S.four_pass_depths(K, seed=K), seed=K), K, 2, npass=4)


def test_frame_patterns_through_the_bucket_form():
    sc = S.frame_pattern_scene()
    forms, three = _check_forms(sc)
    reached = S.check_frame_pattern(three)
    print("bucket form:", {k: len(v) for k, v in sorted(reached.items())})
    assert forms["global"][0] == "buckets", forms


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_far_depths_share_the_last_key_in_id_order_and_infinity_leaves():
    """include/ggr_raster.h, "depth order": any depth below 6.8e37 keeps its exact order; finite depths at or beyond 6.8e37 (6.9e37,
    1e38, 3e38 here) share the last key and are ordered by index among themselves — ids descend with depth in this scene, so
    the DEEPEST comes first; a +inf depth is a non-finite input: radius 0, in no list."""
    sc = S.far_depth_scene()
    forms, three = _check_forms(sc, oracle=False, sync_free=True)
    assert S.check_far(three) >= 1
    for mode in ("per_tile", "global"):
        out, _ = _state(sc, mode)
        S.check_far(out)
    st = oracle_forward(sc)                     # (the oracle orders the last key's Gaussians by depth: only visibility compares)
    assert np.array_equal(three["radii"].cpu().numpy(), st.radii)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_launch_set_where_one_view_meets_the_oversized_bucket():
    """four views of one Gaussian set in one launch set; only view 2 (the scene's own camera) sees the two planes as two keys.
    The fault word is shared by the segments: every view must come out as its own three-pass forward."""
    from ggrt_official_amd.rasterizer import clear_list_hints, debug_forward_state, last_forward_sort_form, rasterize_views
    dev = torch.device("cuda:0")
    sc, vis = _planes(2, 1)
    W, H = sc.width, sc.height
    cams = [camera_matrices(W, H, c2w=p) for p in S.planes_view_poses()]
    s = sc.to(dev)
    ref = []
    for v in (0, 1, 3, 2):
        rs = s.settings()._replace(viewmatrix=cams[v][0].to(dev), projmatrix=cams[v][1].to(dev), campos=cams[v][2].to(dev))
        three = debug_forward_state(s.means3D, s.opacities, rs._replace(depth_sort="global_3pass"), shs=s.shs, cov3D_precomp=s.cov3D)
        assert_lists_in_depth_order(three)
        clear_list_hints()
        buck = debug_forward_state(s.means3D, s.opacities, rs._replace(depth_sort="global"), shs=s.shs, cov3D_precomp=s.cov3D)
        assert last_forward_sort_form() == ("fell_back" if v == 2 else "buckets"), v
        assert_lists_in_depth_order(buck)
        ref.append((v, three))
    clear_list_hints()
    stack = lambda i: torch.stack([c[i] for c in cams]).to(dev)
    tanfov = torch.tensor([[c[3], c[4]] for c in cams], dtype=torch.float32, device=dev)
    with torch.no_grad():
        color, radii, depth = rasterize_views(s.means3D, s.opacities, stack(0), stack(1), stack(2), torch.zeros(4, 3, device=dev),
                                              tanfov, s.settings()._replace(depth_sort="global"), shs=s.shs,
                                              cov3D_precomp=s.cov3D)[:3]
    how = last_forward_sort_form()
    for v, three in ref:
        assert torch.equal(radii[v], three["radii"]), v
        assert torch.equal(color[v], three["color"]), (v, how)
        assert torch.equal(depth[v], three["out_depth"]), (v, how)
    assert how == "fell_back", how


# ---- the order reference over random scenes that so far were compared with another HIP form only ------------------------------
@pytest.mark.parametrize("P,W,H,profile,seed", [(300000, 504, 378, "A", 1), (1100000, 480, 352, "B", 5)])
def test_random_scenes_of_the_bucket_test_are_in_depth_order(P, W, H, profile, seed):
    sc = make_scene(P, W, H, sh_degree=1, profile=profile, seed=seed)
    three, _ = _state(sc, "global_3pass")
    buck, how = _state(sc, "global")
    assert how == "buckets"
    for out in (three, buck):
        assert_lists_in_depth_order(out)
    assert_same_members(buck, three)
