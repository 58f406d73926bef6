"""`splatting.contribution_keep_mask` on hand-made tensors — no GPU."""
import torch

from ggrt_official_amd.splatting import Contributions, contribution_keep_mask


def _c(wmax, count):
    wmax, count = torch.tensor(wmax, dtype=torch.float32), torch.tensor(count, dtype=torch.int32)
    return Contributions(weight_sum=wmax * count, weight_max=wmax, pixel_count=count)


def test_views_are_reduced_with_amax_and_the_thresholds_combine():
    # [v = 2, g = 4]: never seen | seen faintly in one view | seen strongly on few pixels | seen strongly on many
    c = _c([[0.0, 0.01, 0.0, 0.6], [0.0, 0.0, 0.5, 0.2]], [[0, 30, 0, 40], [0, 0, 2, 90]])
    assert contribution_keep_mask(c).tolist() == [False, True, True, True]
    assert contribution_keep_mask(c, min_weight_max=0.1).tolist() == [False, False, True, True]
    assert contribution_keep_mask(c, min_pixel_count=3).tolist() == [False, True, False, True]
    assert contribution_keep_mask(c, min_weight_max=0.1, min_pixel_count=3).tolist() == [False, False, False, True]
    assert contribution_keep_mask(c, min_weight_max=0.6).tolist() == [False, False, False, True]   # (>=, not >)


def test_shapes():
    c3 = _c([[[0.0, 0.3]], [[0.2, 0.0]]], [[[0, 3]], [[2, 0]]])      # [b = 2, v = 1, g = 2] → [b, g]
    m = contribution_keep_mask(c3, min_weight_max=0.1)
    assert m.shape == (2, 2) and m.dtype == torch.bool and m.tolist() == [[False, True], [True, False]]
    c1 = _c([0.0, 0.3], [0, 3])                                        # one call's [g]: as it is
    assert contribution_keep_mask(c1).tolist() == [False, True]
