"""tests/epipolar_encoded_attention_reference.py against the fixtures recorded from the reference's own modules
(tests/golden/epi_attention_enc_*.npz, made by tests/golden/make_epipolar_encoded_attention_golden.py), and against itself:

* the literal restatement (encoding, Linear, add, K and V materialised) in float64 equals the float64 fixtures to 1e-12 relative,
  output and every gradient (x, features, depth, w_enc, b_enc and the attention's weights);
* the folded form (the route of `fused_epipolar_encoded_attention`) in float64 equals the literal one to 1e-12;
* the hand-written backward formulas of the core — what csrc/epipolar_attn_enc.hip computes — pass gradcheck as the backward of
  the core's forward, depth included, and equal autograd to 1e-12;
* the fixtures hold the documented keys, shapes and dtypes, and their inputs are what `make_enc_case` gives for the recorded seed.
No GPU."""
import os

import numpy as np
import pytest
import torch

from tests.epipolar_encoded_attention_reference import (ENC_LEAVES, F, P, enc_core_backward, enc_core_forward, encoded_folded,
                                                        encoded_literal, make_enc_case, positional_encoding, run_enc_route)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name: (N, S, dim, kv_dim, H, D, O, project_out) — as in the generator
SHAPES = {"ten_octaves": (5, 4, 6, 6, 2, 3, 10, True), "one_octave": (3, 8, 8, 5, 4, 2, 1, True), "no_projection": (4, 5, 6, 4, 1, 6, 3, False)}
NAMES = tuple(SHAPES)


def load_enc_golden(name):
    z = np.load(os.path.join(GOLDEN, f"epi_attention_enc_{name}.npz"), allow_pickle=False)
    case = {k: (torch.from_numpy(z[k]) if k in z.files else None) for k in ENC_LEAVES + ("g_out",)}
    case.update(heads=int(z["heads"]), seed=int(z["seed"]), num_octaves=int(z["num_octaves"]))
    return case, z


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def test_the_constants_are_the_float32_roundings():
    assert np.float32(F).view(np.uint32) == 0x40C90FDB and float(np.float32(F)) == F and F != 2 * np.pi
    assert np.float32(P).view(np.uint32) == 0x3FC90FDB and float(np.float32(P)) == P and P != np.pi / 2
    pe = positional_encoding(torch.tensor([0.0, 0.25], dtype=torch.float64), 2)
    assert pe.shape == (2, 4) and float(pe[0, 0]) == 0 and float(pe[0, 2]) == 0 and abs(float(pe[0, 1]) - 1) < 1e-14
    assert abs(float(pe[1, 0]) - np.sin(F * 0.25)) < 1e-15 and abs(float(pe[1, 3]) - np.sin(F * 0.5 + P)) < 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_the_literal_restatement_in_float64_equals_the_reference(name):
    case, z = load_enc_golden(name)
    got = run_enc_route(encoded_literal, case, torch.float64, "cpu")
    assert _rel(got["out"], torch.from_numpy(z["out64"])) <= 1e-12
    for k in ENC_LEAVES:
        if case[k] is None:
            assert k not in got and "g_" + k + "64" not in z.files
            continue
        assert _rel(got[k], torch.from_numpy(z["g_" + k + "64"])) <= 1e-12, k


@pytest.mark.parametrize("name", NAMES)
def test_the_folded_form_in_float64_equals_the_literal_one(name):
    case, _ = load_enc_golden(name)
    lit = run_enc_route(encoded_literal, case, torch.float64, "cpu")
    fold = run_enc_route(encoded_folded, case, torch.float64, "cpu")
    assert set(lit) == set(fold)
    for k in lit:
        assert _rel(fold[k], lit[k]) <= 1e-12, k


def test_the_folded_form_holds_without_a_bias_and_at_one_sample():
    case = make_enc_case(6, 1, 5, 7, 3, 4, 4, 821)
    lit = run_enc_route(encoded_literal, case, torch.float64, "cpu")
    fold = run_enc_route(encoded_folded, case, torch.float64, "cpu")
    for k in lit:
        if k in ("x", "w_q"):       # one sample: the softmax is constant and nothing reaches the query
            assert float(lit[k].abs().max()) == 0 and float(fold[k].abs().max()) <= 1e-14, k
        else:
            assert float(lit[k].abs().max()) > 0 and _rel(fold[k], lit[k]) <= 1e-12, k
    case = make_enc_case(4, 6, 5, 7, 3, 4, 2, 822)
    case["b_enc"] = None
    lit = run_enc_route(encoded_literal, case, torch.float64, "cpu")
    fold = run_enc_route(encoded_folded, case, torch.float64, "cpu")
    assert "b_enc" not in lit and set(lit) == set(fold)
    for k in lit:
        assert _rel(fold[k], lit[k]) <= 1e-12, k


class _EncCore(torch.autograd.Function):
    """enc_core_forward with enc_core_backward as its backward: what the kernels implement"""

    @staticmethod
    def forward(ctx, qk, qe, f, d):
        out_f, out_e, attn = enc_core_forward(qk, qe, f, d)
        ctx.save_for_backward(qk, qe, f, d, attn)
        return out_f, out_e

    @staticmethod
    def backward(ctx, g_f, g_e):
        qk, qe, f, d, attn = ctx.saved_tensors
        return enc_core_backward(qk, qe, f, d, attn, g_f, g_e)


def _core_case(n, s, c, h, o, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    return r(n, h, c), r(n, h, 2 * o), r(n, s, c), torch.rand((n, s), generator=gen, dtype=torch.float64), r(n, h, c), r(n, h, 2 * o)


@pytest.mark.parametrize("n,s,c,h,o", [(3, 5, 4, 2, 2), (2, 1, 3, 1, 1), (1, 7, 1, 3, 3)])
def test_the_backward_formulas_pass_gradcheck_depth_included(n, s, c, h, o):
    qk, qe, f, d, g_f, g_e = _core_case(n, s, c, h, o, n + 10 * s + 100 * c + 1000 * o)
    leaves = [t.requires_grad_(True) for t in (qk, qe, f, d)]
    assert torch.autograd.gradcheck(_EncCore.apply, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("n,s,c,h,o", [(3, 5, 4, 2, 10), (2, 1, 3, 1, 1), (4, 9, 6, 3, 16)])
def test_the_backward_formulas_equal_autograd(n, s, c, h, o):
    qk, qe, f, d, g_f, g_e = _core_case(n, s, c, h, o, 7 + n + 10 * s + 100 * c + 1000 * o)
    leaves = [t.requires_grad_(True) for t in (qk, qe, f, d)]
    out_f, out_e, attn = enc_core_forward(*leaves)
    want = torch.autograd.grad([out_f, out_e], leaves, [g_f, g_e])
    got = enc_core_backward(*[t.detach() for t in leaves], attn.detach(), g_f, g_e)
    for name, a, b in zip(("g_qk", "g_qe", "g_f", "g_d"), got, want):
        if float(b.abs().max()) == 0:       # (s = 1: the softmax of one sample is constant, nothing reaches qk and qe)
            assert s == 1 and name in ("g_qk", "g_qe") and float(a.abs().max()) == 0
        else:
            assert _rel(a, b) <= 1e-12, name


@pytest.mark.parametrize("name", NAMES)
def test_keys_shapes_dtypes_and_seeded_inputs(name):
    case, z = load_enc_golden(name)
    n, s, dim, kv_dim, heads, d, octaves, project_out = SHAPES[name]
    inner = heads * d
    shapes = {"x": (n, 1, dim), "features": (n, s, kv_dim), "depth": (n, s), "w_enc": (kv_dim, 2 * octaves), "b_enc": (kv_dim,),
              "w_q": (inner, dim), "w_kv": (2 * inner, kv_dim)}
    if project_out:
        shapes.update(w_out=(dim, inner), b_out=(dim,))
    else:
        assert heads == 1 and d == dim and case["w_out"] is None and case["b_out"] is None
    assert case["heads"] == heads and case["num_octaves"] == octaves
    want = set(shapes) | {"g_out", "heads", "num_octaves", "seed"} | {p + t for p in ["out"] + ["g_" + k for k in shapes] for t in ("32", "64")}
    assert set(z.files) == want
    assert z["g_out"].shape == (n, 1, dim) and z["g_out"].dtype == np.float64
    assert float(z["depth"].min()) >= 0 and float(z["depth"].max()) <= 1
    for k, shape in shapes.items():
        assert z[k].shape == shape and z[k].dtype == np.float64, k
        for tag, dtype in (("32", np.float32), ("64", np.float64)):
            g = z["g_" + k + tag]
            assert g.shape == shape and g.dtype == dtype and np.isfinite(g).all(), (k, tag)
    for tag, dtype in (("32", np.float32), ("64", np.float64)):
        assert z["out" + tag].shape == (n, 1, dim) and z["out" + tag].dtype == dtype
    again = make_enc_case(n, s, dim, kv_dim, heads, d, octaves, case["seed"], project_out)
    for k in ENC_LEAVES + ("g_out",):
        assert (again[k] is None) == (case[k] is None)
        if again[k] is not None:
            assert torch.equal(again[k], case[k]), k
    for f in z.files:
        assert z[f].dtype in (np.float32, np.float64, np.int64)      # (only arrays of numbers travel)
    assert os.path.getsize(os.path.join(GOLDEN, f"epi_attention_enc_{name}.npz")) <= 24 * 1024
