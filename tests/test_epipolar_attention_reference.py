"""tests/epipolar_attention_reference.py against the fixtures recorded from the reference's own `Attention.forward(x, z)`
(tests/golden/epi_attention_*.npz, made by tests/golden/make_epipolar_attention_golden.py), and against itself:

* the literal restatement (K and V materialised) in float64 equals the fixtures to 1e-12 relative, output and every gradient;
* the folded form (the route of `fused_epipolar_attention`) in float64 equals the literal one to 1e-12;
* the four hand-written backward formulas of the core — what csrc/epipolar_attn.hip computes — pass gradcheck as the backward of
  the core's forward.
No GPU."""
import os

import numpy as np
import pytest
import torch

from tests.epipolar_attention_reference import (WEIGHTS, attention_folded, attention_literal, core_backward, core_forward, make_case,
                                                run_route)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("two_heads", "four_heads", "no_projection")
LEAVES = ("x", "z") + WEIGHTS


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, f"epi_attention_{name}.npz"))
    case = {k: (torch.from_numpy(z[k]) if k in z.files else None) for k in LEAVES + ("g_out",)}
    case.update(heads=int(z["heads"]), seed=int(z["seed"]))
    return case, z


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_the_literal_restatement_in_float64_equals_the_reference(name):
    case, z = load_golden(name)
    got = run_route(attention_literal, case, torch.float64, "cpu")
    assert _rel(got["out"], torch.from_numpy(z["out64"])) <= 1e-12
    for k in LEAVES:
        if case[k] is None:
            assert k not in got and "g_" + k + "64" not in z.files
            continue
        assert _rel(got[k], torch.from_numpy(z["g_" + k + "64"])) <= 1e-12, k
    # and the reference's own float32 run is the float64 one up to float32 rounding
    assert _rel(torch.from_numpy(z["out32"]).double(), torch.from_numpy(z["out64"])) <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_the_folded_form_in_float64_equals_the_literal_one(name):
    case, _ = load_golden(name)
    lit = run_route(attention_literal, case, torch.float64, "cpu")
    fold = run_route(attention_folded, case, torch.float64, "cpu")
    assert set(lit) == set(fold)
    for k in lit:
        assert _rel(fold[k], lit[k]) <= 1e-12, k


def test_the_folded_form_holds_at_large_logits_and_with_a_flat_query():
    for gain in (0.0, 60.0):
        case = make_case(6, 9, 5, 7, 3, 4, 811, q_gain=gain)
        lit = run_route(attention_literal, case, torch.float64, "cpu")
        fold = run_route(attention_folded, case, torch.float64, "cpu")
        for k in lit:
            if float(lit[k].abs().max()) == 0:
                assert float(fold[k].abs().max()) <= 1e-14, k      # (a zero w_q: no gradient reaches the keys)
            else:
                assert _rel(fold[k], lit[k]) <= 1e-11, (gain, k)


class _Core(torch.autograd.Function):
    """core_forward with core_backward as its backward: what the kernels implement"""

    @staticmethod
    def forward(ctx, qk, z):
        out, attn = core_forward(qk, z)
        ctx.save_for_backward(qk, z, attn)
        return out

    @staticmethod
    def backward(ctx, g):
        qk, z, attn = ctx.saved_tensors
        return core_backward(qk, z, attn, g)


@pytest.mark.parametrize("n,s,c,h", [(3, 5, 4, 2), (2, 1, 3, 1), (1, 7, 1, 3)])
def test_the_four_backward_formulas_pass_gradcheck(n, s, c, h):
    gen = torch.Generator().manual_seed(n + 10 * s + 100 * c)
    qk = torch.randn((n, h, c), generator=gen, dtype=torch.float64, requires_grad=True)
    z = torch.randn((n, s, c), generator=gen, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(_Core.apply, (qk, z), eps=1e-6, atol=1e-8, rtol=1e-6)
    g = torch.randn((n, h, c), generator=gen, dtype=torch.float64)
    want = torch.autograd.grad(core_forward(qk, z)[0], [qk, z], g)
    got = core_backward(qk.detach(), z.detach(), core_forward(qk, z)[1].detach(), g)
    for a, b in zip(got, want):
        if float(b.abs().max()) == 0:       # (s = 1: the softmax of one sample is constant, nothing reaches qk)
            assert s == 1 and float(a.abs().max()) == 0
        else:
            assert _rel(a, b) <= 1e-12
