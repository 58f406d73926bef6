"""The torch restatements of GGRt's GRUs (tests/gru_reference.py) against fixtures made by the reference's own `SepConvGRU` and
`ConvGRU` (tests/golden/make_gru_golden.py), in float64 on the CPU: the literal form equals the fixtures to 1e-12, the split form
equals the literal one to 1e-12 on the output and on every gradient, the checkpoint conversion of `FusedSepConvGRU` /
`FusedConvGRU` is the identity to the bit both ways, and the four backward formulas of the kernels pass gradcheck.  Also the shapes
the GPU tests run (`GPU_SHAPES`)."""
import glob
import os

import numpy as np
import pytest
import torch

from ggrt_official_amd import FusedConvGRU, FusedSepConvGRU
from tests.gru_reference import (HALVES, blend_backward, blend_forward, gate_backward, gate_forward, make_gru_case, reference_keys, result_keys, run_gru,
                                 split_names, split_params)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f)[len("gru_"):-4] for f in glob.glob(os.path.join(GOLDEN, "gru_*.npz")))
MODULES = {"sep": FusedSepConvGRU, "conv": FusedConvGRU}

# (N, Ch, Cx, H, W, seed): M = Ch H W is odd in the first two (the 4-byte path; the second has the n 2M block offsets), a multiple
# of 4 in the third (16-byte path, the fixtures' shape); the fourth has 3105 elements, neither a multiple of 256 nor of 4, over
# several workgroups; the last two are GGRt's depth block and its pose block in lock-step over five views
GPU_SHAPES = {
    "1x3x3x5": (1, 3, 2, 3, 5, 1010),
    "2x3x3x5": (2, 3, 2, 3, 5, 1011),
    "2x4x5x7": (2, 4, 6, 5, 7, 1012),
    "3x5x9x23": (3, 5, 3, 9, 23, 1013),
    "1x128x48x63": (1, 128, 160, 48, 63, 1014),
    "5x128x48x63": (5, 128, 160, 48, 63, 1015),
}


def _load(name):
    z = np.load(os.path.join(GOLDEN, f"gru_{name}.npz"), allow_pickle=False)
    kind = name.split("_")[0]
    case = dict(sd={k: torch.from_numpy(z["sd." + k]) for k in reference_keys(kind)}, h=torch.from_numpy(z["h"]), x=torch.from_numpy(z["x"]),
                g=torch.from_numpy(z["g"]))
    return z, kind, case


def test_there_are_four_fixtures_of_the_shapes_the_issue_names():
    assert FIXTURES == ["conv_n1_c3", "conv_n2_c4", "sep_n1_c3", "sep_n2_c4"]
    for n in FIXTURES:
        z, kind, case = _load(n)
        want = ((2, 4, 5, 7), (2, 6, 5, 7)) if n.endswith("n2_c4") else ((1, 3, 3, 5), (1, 2, 3, 5))
        assert (tuple(case["h"].shape), tuple(case["x"].shape)) == want and z["out"].dtype == np.float64
        assert os.path.getsize(os.path.join(GOLDEN, f"gru_{n}.npz")) < 64 * 1024          # (float64 noise does not compress: 12 to 40 KiB)


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_literal_restatement_equals_the_reference(name):
    z, kind, case = _load(name)
    got = run_gru("literal", kind, case, torch.float64, "cpu")
    want = split_params(kind, {k: torch.from_numpy(z["g_sd." + k]) for k in reference_keys(kind)}, case["h"].shape[1])
    np.testing.assert_allclose(got["out"].numpy(), z["out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["g_h"].numpy(), z["g_h"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["g_x"].numpy(), z["g_x"], rtol=0, atol=1e-12)
    for k in split_names(kind):
        np.testing.assert_allclose(got["g_" + k].numpy(), want[k].numpy(), rtol=0, atol=1e-12, err_msg=k)
    assert float(np.abs(z["g_sd.convr" + HALVES[kind][0][0] + ".weight"]).max()) > 1e-3          # (the r gate is live)


@pytest.mark.parametrize("name", FIXTURES)
def test_split_form_equals_the_literal_one(name):
    _, kind, case = _load(name)
    lit, spl = run_gru("literal", kind, case, torch.float64, "cpu"), run_gru("split", kind, case, torch.float64, "cpu")
    for k in result_keys(kind):
        np.testing.assert_allclose(spl[k].numpy(), lit[k].numpy(), rtol=0, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("kind", sorted(MODULES))
def test_checkpoint_conversion_is_the_identity_to_the_bit(kind):
    ch, cx = 5, 3
    case = make_gru_case(kind, 1, ch, cx, 2, 2, 1020)
    sd = {k: v.float() for k, v in case["sd"].items()}
    m = MODULES[kind](ch, cx)
    assert sorted(n for n, _ in m.named_parameters()) == sorted(split_names(kind))
    m.load_reference_state_dict(sd)
    back = m.reference_state_dict()
    assert list(back) == reference_keys(kind)
    for k in sd:
        assert back[k].dtype == torch.float32 and torch.equal(back[k], sd[k]), k
    want = split_params(kind, sd, ch)
    for k, v in m.named_parameters():
        assert torch.equal(v.detach(), want[k]), k
    # ... and the other way: a freshly initialised module -> the reference's keys -> a second module
    m2, m3 = MODULES[kind](ch, cx), MODULES[kind](ch, cx)
    m3.load_reference_state_dict(m2.reference_state_dict())
    for (k, a), (_, b) in zip(m2.named_parameters(), m3.named_parameters()):
        assert torch.equal(a, b) and float(a.detach().abs().max()) > 0, k
    with pytest.raises(ValueError, match="expected the keys"):
        m.load_reference_state_dict({k: v for k, v in sd.items() if not k.endswith("bias")})
    bad = dict(sd)
    bad[reference_keys(kind)[0]] = bad[reference_keys(kind)[0]][:, :-1]
    with pytest.raises(ValueError, match="has weight"):
        m.load_reference_state_dict(bad)


def test_reference_modules_take_the_converted_state_dict():
    """nn.Conv2d layers laid out as the reference's modules accept `reference_state_dict()` strictly."""
    for kind, cls in MODULES.items():
        ch, cx = 4, 6
        m = cls(ch, cx)
        holder = torch.nn.Module()
        for s, k, pad in HALVES[kind]:
            for gate in "zrq":
                setattr(holder, f"conv{gate}{s}", torch.nn.Conv2d(ch + cx, ch, k, padding=pad))
        holder.load_state_dict(m.reference_state_dict(), strict=True)


def test_the_four_backward_formulas_pass_gradcheck():
    gen = torch.Generator().manual_seed(1030)
    N, ch, H, W = 2, 3, 2, 3
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    a_zr_h, a_zr_x, h, a_q_h, a_q_x = rnd(N, 2 * ch, H, W), rnd(N, 2 * ch, H, W), torch.tanh(rnd(N, ch, H, W)), rnd(N, ch, H, W), rnd(N, ch, H, W)

    class Gate(torch.autograd.Function):
        """(z, rh) with the gradient slot of z carrying dL/da_z, as the kernels pass it"""
        @staticmethod
        def forward(ctx, a_h, a_x, hh):
            z, r, rh = gate_forward(a_h, a_x, hh)
            ctx.save_for_backward(r, hh)
            return z, rh

        @staticmethod
        def backward(ctx, g_a_z, g_rh):
            r, hh = ctx.saved_tensors
            g_a_r, g_h = gate_backward(g_rh, hh, r)
            g_a = torch.cat([g_a_z, g_a_r], 1)
            return g_a, g_a, g_h

    class Blend(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a_h, a_x, z, hh):
            q, out = blend_forward(a_h, a_x, z, hh)
            ctx.save_for_backward(z, q, hh)
            return out

        @staticmethod
        def backward(ctx, g):
            z, q, hh = ctx.saved_tensors
            g_a_q, g_a_z, g_h = blend_backward(g, z, q, hh)
            return g_a_q, g_a_q, g_a_z, g_h

    def step(a_h, a_x, hh, b_h, b_x, w):
        z, rh = Gate.apply(a_h, a_x, hh)
        return Blend.apply(b_h + w * rh, b_x, z, hh)          # (w * rh stands for the w_q_h convolution)

    args = [t.clone().requires_grad_(True) for t in (a_zr_h, a_zr_x, h, a_q_h, a_q_x)] + [rnd(1, ch, 1, 1).requires_grad_(True)]
    assert torch.autograd.gradcheck(step, args, eps=1e-6, atol=1e-8, rtol=1e-6)
    # the fused h gradient of the gate: dL/dh_part + dL/drh r
    g_rh, part = rnd(N, ch, H, W), rnd(N, ch, H, W)
    r = torch.sigmoid(rnd(N, ch, H, W))
    assert torch.equal(gate_backward(g_rh, h, r, part)[1], part + g_rh * r) and torch.equal(gate_backward(g_rh, h, r, part)[0], gate_backward(g_rh, h, r)[0])


def test_the_gpu_shapes_are_the_regimes_their_comments_claim():
    M = {k: v[1] * v[3] * v[4] for k, v in GPU_SHAPES.items()}
    assert M["1x3x3x5"] % 4 and M["2x3x3x5"] % 4 and M["2x4x5x7"] % 4 == 0 and M["1x128x48x63"] % 4 == 0
    n = GPU_SHAPES["3x5x9x23"][0] * M["3x5x9x23"]
    assert n % 4 and n % 256 and n > 4 * 256
    assert all(v[2] == 160 for k, v in GPU_SHAPES.items() if "128" in k)
