"""The order reference of the depth-sort tests (tests/helpers.py: sort_key, assert_lists_in_depth_order, assert_same_members)
proved on the C oracle's lists — accepted as they are, rejected after each of three corruptions — and the precondition of every
adversarial scene of tests/sort_scenes.py checked with the oracle for visibility.  No GPU."""
import copy

import numpy as np
import pytest

from ggrt_official_amd.synthetic import make_scene
from tests import sort_scenes as S
from tests.helpers import (assert_lists_in_depth_order, assert_same_members, oracle_forward, order_state, sort_key)


def _tied_planes(P=6000):
    sc = make_scene(P, 160, 128, sh_degree=0, profile="A", seed=5)
    return S.at_depths(sc, 4.0 + (np.arange(P) % 3).astype(np.float32))


def test_sort_key_is_the_header_rule():
    d = np.array([0.2, np.nextafter(np.float32(0.2), np.float32(1)), 1.0, 6.7e37, 6.81e37, 6.9e37, 3e38, np.inf], np.float32)   # (the clamp sits at 6.8056e37)
    k = sort_key(d)
    assert k[0] == 0 and k[1] == 1 and k[2] == 0x3F800000 - 0x3E4CCCCD
    assert k[3] < 0x3FFFFFFF and (k[4:] == 0x3FFFFFFF).all()
    assert (np.diff(k[:5].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("scene", ["random", "tied"])
def test_checker_accepts_the_oracle_and_rejects_three_corruptions(scene):
    sc = make_scene(8000, 160, 128, sh_degree=0, profile="A", seed=1) if scene == "random" else _tied_planes()
    st = oracle_forward(sc)
    assert_lists_in_depth_order(st)
    assert_same_members(st, st)
    s = order_state(st)
    key, pl, rg = sort_key(s["depth"]), s["point_list"], s["ranges"]
    inside = np.ones(len(pl) - 1, bool)                      # entry i and i + 1 in one tile
    inside[rg[rg[:, 0] > 0, 0] - 1] = False
    diff_key = np.flatnonzero(inside & (key[pl[:-1]] != key[pl[1:]]))
    same_key = np.flatnonzero(inside & (key[pl[:-1]] == key[pl[1:]]))
    assert len(diff_key)
    if scene == "tied":
        assert len(same_key) > 100

    def corrupted(i):
        bad = copy.copy(st)
        bad.point_list = st.point_list.copy()
        bad.point_list[[i, i + 1]] = bad.point_list[[i + 1, i]]
        return bad
    # (a) two neighbours of different keys swapped
    with pytest.raises(AssertionError, match="out of"):
        assert_lists_in_depth_order(corrupted(int(diff_key[len(diff_key) // 2])))
    assert_same_members(st, corrupted(int(diff_key[0])))     # (membership is not the order's business)
    # (b) two neighbours of EQUAL key swapped: descending id
    if len(same_key):
        with pytest.raises(AssertionError, match="out of"):
            assert_lists_in_depth_order(corrupted(int(same_key[len(same_key) // 2])))
    # (c) one id moved to another tile: the ranges shift by one entry, the list keeps its length
    lens = rg[:, 1] - rg[:, 0]
    t = int(np.flatnonzero((lens[:-1] > 1) & (lens[1:] > 0))[0])
    moved = copy.copy(st)
    moved.ranges = st.ranges.copy()
    moved.ranges[t, 1] -= 1
    moved.ranges[t + 1, 0] -= 1
    with pytest.raises(AssertionError):
        assert_same_members(st, moved)
    # … or, with the ranges kept, an entry of a tile replaced by a Gaussian that is not in it
    other = copy.copy(st)
    other.point_list = st.point_list.copy()
    other.point_list[rg[t, 0]] = np.setdiff1d(np.flatnonzero(s["radii"] > 0), pl[rg[t, 0]:rg[t, 1]])[0]
    with pytest.raises(AssertionError):
        assert_same_members(st, other)


@pytest.mark.parametrize("period,gap", [(2, 1), (4, 1), (64, 1), (256, 1), (3, 1), (2, 100)])
def test_interleaved_planes_are_adversarial(period, gap):
    vis = oracle_forward(S.interleaved_planes_scene(period)).radii > 0
    assert 0 < (~vis[:20000]).sum()                          # (some are culled: id parity is not bucket-position parity)
    st = oracle_forward(S.interleaved_planes_scene(period, gap, visible=vis))
    assert S.check_interleaved(st, period, vis) >= 100       # tiles that hold both planes
    assert_lists_in_depth_order(st)


def test_route_model_on_hand_made_keys():
    m = S.route_model
    assert m([7, 7, 7])["route"] == 0
    assert m([0x100, 0x101]) == dict(route=1, nbits=1, npass=1, digit=1)
    assert m([0] * 25 + [1]) == dict(route=2, nbits=1, npass=1, digit=1)
    assert m([0] * 24 + [1])["route"] == 1
    assert m([0] * 30 + [(1 << 19) - 1]) == dict(route=2, nbits=19, npass=3, digit=7)
    assert m([0] * 30 + [(1 << 27)]) == dict(route=2, nbits=28, npass=4, digit=7)
    # the bits that differ against the range: 0x0FF and 0x100 differ in nine bits and lie one apart
    assert m([0xFF] * 30 + [0x100])["nbits"] == 9 and m([0xFF] * 30 + [0x100], rel=True)["nbits"] == 1


@pytest.mark.parametrize("route,nbits,K", S.one_tile_cases())
def test_bit_patterns_reach_the_branch_they_are_named_for(route, nbits, K):
    st = oracle_forward(S.one_tile_scene(S.pattern_depths(S.key_pattern(route, nbits, K, seed=K)), seed=K))
    m = S.check_one_tile(st, K, route, nbits=nbits)
    if route == 2:
        assert m["npass"] == -(-nbits // 9) and m["digit"] == -(-nbits // m["npass"])
        assert S.tile_routes(st)[1] >= K
    assert_lists_in_depth_order(st)


def test_every_class_meets_every_kind_of_branch():
    kinds = {}
    for route, nbits, K in S.one_tile_cases():
        q = 8 if K <= 2048 else 12 if K <= 3072 else 16 if K <= 4096 else 32
        npass = -(-nbits // 9)
        kinds.setdefault(q, set()).add((route, route == 2 and -(-nbits // npass) > 6))
    assert all(kinds[q] == {(1, False), (2, False), (2, True)} for q in (8, 12, 16, 32)), kinds
    assert {nb for r, nb, _ in S.one_tile_cases() if r == 1} == {1, 9, 10, 18, 22}
    assert {nb for r, nb, _ in S.one_tile_cases() if r == 2} == set(S.ROUTE2_NBITS)


def test_four_pass_pattern():
    st = oracle_forward(S.one_tile_scene(S.four_pass_depths(3000), seed=1))
    assert S.check_one_tile(st, 3000, 2, npass=4)["nbits"] >= 28
    assert_lists_in_depth_order(st)


def test_frame_patterns_reach_the_routes_of_the_bucket_form():
    st = oracle_forward(S.frame_pattern_scene())
    assert 30000 <= st.P <= 150000
    S.check_frame_pattern(st)
    assert_lists_in_depth_order(st)


def test_far_depths_on_the_oracle():
    """visibility is the product's (finite depths stay, +inf leaves); the oracle sorts on the full float bits — it does not give
    the depths at or beyond 6.8e37 one key — and the checker, which does, says so"""
    st = oracle_forward(S.far_depth_scene())
    S.check_far(st, lists=False)
    with pytest.raises(AssertionError, match="out of"):
        assert_lists_in_depth_order(st)
