"""The fused epipolar cross-attention (csrc/epipolar_attn.hip, `fused_epipolar_attention`, `epipolar_attention_core`) against the
literal restatement of the reference's `Attention.forward(x, z)` (tests/epipolar_attention_reference.py), forward and backward.

Three routes: the literal restatement (K and V materialised) in float64 on the CPU (`ref`), the same in float32 on the device
(`t32`), `fused_epipolar_attention` (`ker`).  For the output and for every gradient (x, z, w_q, w_kv, w_out, b_out)
e = max|x − ref64| / max|ref64|  and the bar is  e_kernel <= max(4·e_torch32, 1e-6).  The upstream gradient is fixed and random.

Shapes: the smallest at which the kernels can go wrong.  A workgroup is ONE wave and owns one ray, so N only sets the grid:
N = 1, 3, 4, 5, 257.  Lane s owns sample s in the row phase (logits, softmax, dl): S = 1, 2, 31, 32, 33, 64 walk the lane mask
through one lane, half a wave ± 1 and the full wave.  The tile is loaded with 16-byte loads when C is a multiple of 4 and
element by element otherwise, the row phase reads it in float4 steps with a partial last step, and the column phase walks the
channels in trips of 64 lanes: C = 1, 3 (one partial float4), 64 (one full trip), 127 and 130 (element loads, partial float4,
partial trip), 128, 256 (two and four full trips).  H = 1, 3, 4, 8 walk the per-lane accumulators up to their bound.  S = 64 with
C = 256 is the one tile above 64 KiB of LDS (the kernels ask for the larger limit there).  Everything else is small (dim <= 8,
D <= 4) except the case at GGRt's own S = 32, C = 128, H = 4, D = 128."""
import pytest
import torch

from tests.epipolar_attention_reference import attention_literal, core_backward, core_forward, make_case, run_route

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _routes(n, s, dim, c, h, d, project_out=True, q_gain=1.0):
    key = (n, s, dim, c, h, d, project_out, q_gain)
    if key not in _CACHE:
        from ggrt_official_amd import fused_epipolar_attention
        case = make_case(n, s, dim, c, h, d, 3 * n + 5 * s + 7 * dim + 11 * c + 13 * h + 17 * d, project_out, q_gain)
        _CACHE[key] = (case, run_route(attention_literal, case, torch.float64, "cpu"), run_route(attention_literal, case, torch.float32, DEV),
                       run_route(fused_epipolar_attention, case, torch.float32, DEV))
    return _CACHE[key]


def _err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def _hold_to_the_bar(ref, t32, ker, what="", may_be_zero=()):
    assert set(ker) == set(ref) == set(t32)
    bad = []
    for k, r in ref.items():
        assert ker[k].shape == r.shape, (k, ker[k].shape, r.shape)
        assert bool(torch.isfinite(ker[k]).all()), k
        if float(r.abs().max()) == 0:
            assert k in may_be_zero and float(ker[k].abs().max()) == 0, k
            continue
        e_k, e_t = _err(ker[k], r), _err(t32[k], r)
        print(f"{what} {k:6s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad


SAMPLES = [(5, s, 6, 5, 2, 3) for s in (1, 2, 31, 32, 33, 64)]
CHANNELS = [(3, 5, 6, c, 3, 2) for c in (1, 3, 64, 127, 128, 130, 256)]
HEADS = [(4, 7, 8, 12, h, 4) for h in (1, 3, 4, 8)]
RAYS = [(n, 8, 6, 16, 2, 3) for n in (1, 3, 4, 5, 257)]
OTHERS = [(64, 32, 128, 128, 4, 128),       # GGRt's own layer
          (2, 64, 6, 256, 8, 2),            # the largest tile: 66 560 bytes of LDS
          (3, 33, 5, 130, 8, 1)]


@pytest.mark.parametrize("n,s,dim,c,h,d", SAMPLES + CHANNELS + HEADS + RAYS + OTHERS)
def test_output_and_every_gradient_match_the_float64_restatement(n, s, dim, c, h, d):
    case, ref, t32, ker = _routes(n, s, dim, c, h, d)
    assert ref["out"].shape == (n, 1, dim) and ref["z"].shape == (n, s, c)
    # one sample: the softmax is constant, and nothing reaches the query or the keys
    _hold_to_the_bar(ref, t32, ker, f"N={n} S={s} dim={dim} C={c} H={h} D={d}", may_be_zero=("x", "w_q") if s == 1 else ())


def test_one_head_of_full_width_has_no_output_projection_and_x_may_be_two_dimensional():
    case, ref, t32, ker = _routes(5, 9, 6, 7, 1, 6, project_out=False)
    assert "w_out" not in ker and "b_out" not in ker
    _hold_to_the_bar(ref, t32, ker, "no projection")
    from ggrt_official_amd import fused_epipolar_attention
    flat = run_route(lambda x, *a: fused_epipolar_attention(x.reshape(5, 6), *a).reshape(5, 1, 6), case, torch.float32, DEV)
    for k in ker:
        assert torch.equal(flat[k], ker[k]), k
    args = [case[k].to(device=DEV, dtype=torch.float32) for k in ("x", "z", "w_q", "w_kv")]
    out, weights = fused_epipolar_attention(*args, None, None, 1, return_weights=True)
    assert out.shape == (5, 1, 6) and weights.shape == (5, 1, 9) and not weights.requires_grad
    with pytest.raises(ValueError, match="ONE query token per ray"):
        fused_epipolar_attention(args[0].expand(5, 2, 6), *args[1:], None, None, 1)
    with pytest.raises(RuntimeError, match="outside 1..64"):
        fused_epipolar_attention(args[0], args[1].repeat(1, 8, 1), *args[2:], None, None, 1)      # 72 samples


def test_large_logits_stay_finite_and_hold_the_bar():
    n, s, dim, c, h, d = 16, 16, 6, 16, 2, 3
    case, ref, t32, ker = _routes(n, s, dim, c, h, d, q_gain=40.0)
    q = (case["x"].reshape(n, dim) @ case["w_q"].t()).reshape(n, h, d)
    k = (case["z"] @ case["w_kv"][:h * d].t()).reshape(n, s, h, d)
    logits = torch.einsum("nhd,nshd->nhs", q, k) * d ** -0.5
    assert float(logits.max()) >= 80 and float(logits.min()) <= -80, (float(logits.min()), float(logits.max()))
    _hold_to_the_bar(ref, t32, ker, "large logits")


def _core_inputs(n, s, c, h, seed):
    gen = torch.Generator().manual_seed(seed)
    qk = torch.randn((n, h, c), generator=gen, dtype=torch.float64)
    z = torch.randn((n, s, c), generator=gen, dtype=torch.float64)
    return qk, z, torch.randn((n, h, c), generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("s", [1, 3, 7, 32, 33, 64])
def test_rows_of_attn(s):
    from ggrt_official_amd import epipolar_attention_core
    n, c, h = 5, 20, 3
    qk, z, _ = _core_inputs(n, s, c, h, 40 + s)
    qk32, z32 = qk.to(device=DEV, dtype=torch.float32), z.to(device=DEV, dtype=torch.float32)
    ctx, attn = epipolar_attention_core(qk32 * 3, z32)
    assert attn.shape == (n, h, s) and not attn.requires_grad and bool((attn >= 0).all())
    assert float((attn.double().sum(-1) - 1).abs().max()) <= 1e-6
    # qk = 0: exp(0) = 1 and the sum s are exact, so every weight is 1/s rounded once
    ctx0, attn0 = epipolar_attention_core(torch.zeros_like(qk32), z32)
    exact = torch.tensor(1.0 / s, dtype=torch.float64)
    assert float((attn0.double() - exact).abs().max()) <= 2.0 ** -24 * float(exact)
    assert _err(ctx0.double().cpu(), z.to(torch.float32).double().mean(1, keepdim=True).expand(n, h, c)) <= 1e-6
    # all samples of a ray equal: whatever the weights, ctx is that sample
    same = z32[:, :1].expand(n, s, c).contiguous()
    ctx1, _ = epipolar_attention_core(qk32 * 3, same)
    assert _err(ctx1.double().cpu(), same[:, :1].expand(n, h, c).double().cpu()) <= 1e-6


def test_the_core_matches_its_float64_formulas():
    """the kernels alone, without the projections around them: ctx, attn, g_qk and g_z against core_forward / core_backward"""
    from ggrt_official_amd import epipolar_attention_core
    qk, z, g = _core_inputs(7, 33, 68, 5, 51)
    qk = qk * 0.3
    ctx64, attn64 = core_forward(qk, z)
    gqk64, gz64 = core_backward(qk, z, attn64, g)
    qk32 = qk.to(device=DEV, dtype=torch.float32).requires_grad_(True)
    z32 = z.to(device=DEV, dtype=torch.float32).requires_grad_(True)
    ctx, attn = epipolar_attention_core(qk32, z32)
    gqk, gz = torch.autograd.grad(ctx, [qk32, z32], g.to(device=DEV, dtype=torch.float32))
    # float32 against float64 on the same formulas.  The worst case of a 68-term float32 dot product is 68·2^-24·Σ|q_c||z_c|, about
    # 4e-6 · 68·0.3·0.64 = 5e-5 on a logit, which is the relative error of a weight; the gradients stack two such sums
    for name, got, want in (("ctx", ctx, ctx64), ("attn", attn, attn64), ("g_qk", gqk, gqk64), ("g_z", gz, gz64)):
        e = _err(got.detach().double().cpu(), want)
        print(f"core {name:5s} e {e:.3e}")
        assert e <= 2e-4, (name, e)


def test_forward_and_backward_give_the_same_bits_twice():
    from ggrt_official_amd import epipolar_attention_core
    qk, z, g = _core_inputs(257, 32, 128, 4, 52)
    g32 = g.to(device=DEV, dtype=torch.float32)
    runs = []
    for _ in range(2):
        qk32 = qk.to(device=DEV, dtype=torch.float32).requires_grad_(True)
        z32 = z.to(device=DEV, dtype=torch.float32).requires_grad_(True)
        ctx, attn = epipolar_attention_core(qk32, z32)
        runs.append((ctx.detach(), attn) + torch.autograd.grad(ctx, [qk32, z32], g32))
    assert float(runs[0][2].abs().max()) > 0 and float(runs[0][3].abs().max()) > 0
    for a, b, name in zip(runs[0], runs[1], ("ctx", "attn", "g_qk", "g_z")):
        assert torch.equal(a, b), name


def test_memory_stays_below_twice_the_bytes_of_z():
    """K and V alone would be 2·H·D/C = 8 × the bytes of z; the fused route needs g_z (1 ×) plus [N,H,C]- and [N,H·D]-sized
    tensors (1/8 of z each at this shape).  Derived, not measured: the rise of the peak over a forward + backward, above what is
    allocated once the inputs exist, is at most 2 × the bytes of z."""
    from ggrt_official_amd import fused_epipolar_attention
    n, s, c, h, d, dim = 1024, 32, 128, 4, 128, 128
    case = make_case(n, s, dim, c, h, d, 53)
    names = ("x", "z", "w_q", "w_kv", "w_out", "b_out")

    def step(rays):
        leaf = [case[k][:rays].clone() if k in ("x", "z") else case[k].clone() for k in names]
        leaf = [t.to(device=DEV, dtype=torch.float32).requires_grad_(True) for t in leaf]
        g = case["g_out"][:rays].to(device=DEV, dtype=torch.float32)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fused_epipolar_attention(*leaf, h)
        out.backward(g)
        torch.cuda.synchronize()
        assert leaf[1].grad is not None and leaf[1].grad.shape == leaf[1].shape
        return torch.cuda.max_memory_allocated() - before, leaf[1].numel() * 4

    step(8)      # (the BLAS library's workspace and the code objects exist from here on)
    rise, z_bytes = step(n)
    print(f"rise of the peak {rise / 2 ** 20:.2f} MiB, z {z_bytes / 2 ** 20:.2f} MiB, ratio {rise / z_bytes:.3f}")
    assert z_bytes == n * s * c * 4 and rise <= 2 * z_bytes, (rise, z_bytes)


def test_element_offsets_past_two_to_the_31():
    """N·S·C = 2^31 + 8·2^14 floats: the last rays lie past a 32-bit element offset.  They must equal, to the bit, the same rays
    computed on their own (N = 8), forward and backward."""
    from ggrt_official_amd import epipolar_attention_core
    s, c, h = 64, 256, 1
    n = (1 << 31) // (s * c) + 8
    z = torch.empty((n, s, c), dtype=torch.float32, device=DEV).normal_(generator=torch.Generator(DEV).manual_seed(54))
    qk = torch.empty((n, h, c), dtype=torch.float32, device=DEV).normal_(generator=torch.Generator(DEV).manual_seed(55)) * 0.2
    g = torch.empty((n, h, c), dtype=torch.float32, device=DEV).normal_(generator=torch.Generator(DEV).manual_seed(56))
    z.requires_grad_(True)
    qk.requires_grad_(True)
    ctx, attn = epipolar_attention_core(qk, z)
    g_qk, g_z = torch.autograd.grad(ctx, [qk, z], g)
    tail_z, tail_qk = z.detach()[-8:].clone().requires_grad_(True), qk.detach()[-8:].clone().requires_grad_(True)
    ctx_t, attn_t = epipolar_attention_core(tail_qk, tail_z)
    g_qk_t, g_z_t = torch.autograd.grad(ctx_t, [tail_qk, tail_z], g[-8:].clone())
    assert float(ctx_t.detach().abs().max()) > 0 and float(g_z_t.abs().max()) > 0
    for a, b, name in ((ctx[-8:], ctx_t, "ctx"), (attn[-8:], attn_t, "attn"), (g_qk[-8:], g_qk_t, "g_qk"), (g_z[-8:], g_z_t, "g_z")):
        assert torch.equal(a.detach(), b.detach()), name
