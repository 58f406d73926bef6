"""The epipolar cross-attention with the depth encoding folded in (csrc/epipolar_attn_enc.hip, `fused_epipolar_encoded_attention`,
`epipolar_encoded_attention_core`) against the literal restatement of the reference — PositionalEncoding, Linear, add, then
`Attention.forward(x, z)` (tests/epipolar_encoded_attention_reference.py) — forward and backward.

Three routes: the literal restatement in float64 on the CPU (`ref`), the same in float32 on the device (`t32`),
`fused_epipolar_encoded_attention` (`ker`).  For the output and for every gradient (x, features, depth, w_enc, b_enc, w_q, w_kv,
w_out, b_out)  e = max|x − ref64| / max|ref64|  and the bar is  e_kernel <= max(4·e_torch32, 1e-6).  The upstream gradient is
fixed and random; the depths are float32 numbers in [0, 1], the same in every route.

Shapes: the smallest at which the kernels can go wrong.  A workgroup is ONE wave and owns one ray, so N only sets the grid:
N = 1, 3, 257.  Lane s owns sample s in the row phase, and the S·O sines are spread over 64 / 2^⌈log2 S⌉ groups of lanes:
S = 1, 2, 31, 32, 33, 64 walk the lane mask and the groups (64, 32, 2, 2, 1, 1 of them).  C = 1, 3, 64, 127, 128, 130, 256 walk
the vector and the element loads, the partial float4 and the trips of the column phase, in which the encoding's E columns follow
the C channels (so C + E crosses a multiple of 64 in several of them).  H = 1, 3, 4, 8 walk the accumulators.  O = 1, 2, 3, 10,
16 give E = 2, 4, 6, 20, 32: partial and full float4s of the encoding, and the highest octave.  S = 64 with C = 256 and O = 16 is
the largest tile, 74 752 bytes of LDS (the kernels ask for the larger limit there).  Everything else is small (dim <= 8, D <= 4)
except the case at GGRt's own S = 32, C = 128, H = 4, D = 128, O = 10."""
import pytest
import torch

from tests.epipolar_encoded_attention_reference import (ENC_LEAVES, enc_core_backward, enc_core_forward, encoded_literal, make_enc_case,
                                                        positional_encoding, run_enc_route)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _routes(n, s, dim, c, h, d, o, project_out=True):
    key = (n, s, dim, c, h, d, o, project_out)
    if key not in _CACHE:
        from ggrt_official_amd import fused_epipolar_encoded_attention
        case = make_enc_case(n, s, dim, c, h, d, o, 3 * n + 5 * s + 7 * dim + 11 * c + 13 * h + 17 * d + 19 * o, project_out)
        _CACHE[key] = (case, run_enc_route(encoded_literal, case, torch.float64, "cpu"), run_enc_route(encoded_literal, case, torch.float32, DEV),
                       run_enc_route(fused_epipolar_encoded_attention, case, torch.float32, DEV))
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
        print(f"{what} {k:8s} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        if not (e_k <= max(4 * e_t, 1e-6)):
            bad.append((k, e_k, e_t))
    assert not bad, bad


SAMPLES = [(5, s, 6, 5, 2, 3, 3) for s in (1, 2, 31, 32, 33, 64)]
CHANNELS = [(3, 5, 6, c, 3, 2, 2) for c in (1, 3, 64, 127, 128, 130, 256)]
HEADS = [(4, 7, 8, 12, h, 4, 3) for h in (1, 3, 4, 8)]
OCTAVES = [(4, 7, 6, 9, 2, 3, o) for o in (1, 2, 3, 10, 16)]
RAYS = [(n, 8, 6, 16, 2, 3, 2) for n in (1, 3, 257)]
OTHERS = [(64, 32, 128, 128, 4, 128, 10),      # GGRt's own layer
          (2, 64, 6, 256, 8, 2, 16),           # the largest tile: 74 752 bytes of LDS
          (3, 33, 5, 130, 8, 1, 5)]


@pytest.mark.parametrize("n,s,dim,c,h,d,o", SAMPLES + CHANNELS + HEADS + OCTAVES + RAYS + OTHERS)
def test_output_and_every_gradient_match_the_float64_restatement(n, s, dim, c, h, d, o):
    case, ref, t32, ker = _routes(n, s, dim, c, h, d, o)
    assert set(ref) == set(ENC_LEAVES) | {"out"}
    assert ref["out"].shape == (n, 1, dim) and ref["features"].shape == (n, s, c) and ref["depth"].shape == (n, s) and ref["w_enc"].shape == (c, 2 * o)
    # one sample: the softmax is constant and nothing reaches the query or the keys — but the value path carries the encoding
    _hold_to_the_bar(ref, t32, ker, f"N={n} S={s} dim={dim} C={c} H={h} D={d} O={o}", may_be_zero=("x", "w_q") if s == 1 else ())
    if s == 1:
        for k in ("x", "w_q"):
            assert float(ref[k].abs().max()) == 0 and float(ker[k].abs().max()) == 0, k
        for k in ("w_enc", "b_enc", "depth", "features"):
            assert float(ref[k].abs().max()) > 0 and float(ker[k].abs().max()) > 0, k


def test_no_output_projection_no_bias_and_a_two_dimensional_x():
    case, ref, t32, ker = _routes(5, 9, 6, 7, 1, 6, 3, project_out=False)
    assert "w_out" not in ker and "b_out" not in ker
    _hold_to_the_bar(ref, t32, ker, "no projection")
    from ggrt_official_amd import fused_epipolar_encoded_attention
    flat = run_enc_route(lambda x, *a: fused_epipolar_encoded_attention(x.reshape(5, 6), *a).reshape(5, 1, 6), case, torch.float32, DEV)
    for k in ker:
        assert torch.equal(flat[k], ker[k]), k
    nobias = dict(case, b_enc=None)
    _hold_to_the_bar(run_enc_route(encoded_literal, nobias, torch.float64, "cpu"), run_enc_route(encoded_literal, nobias, torch.float32, DEV),
                     run_enc_route(fused_epipolar_encoded_attention, nobias, torch.float32, DEV), "no bias")
    args = [case[k].to(device=DEV, dtype=torch.float32) for k in ENC_LEAVES[:7]]
    out, weights = fused_epipolar_encoded_attention(*args, None, None, 1, return_weights=True)
    assert out.shape == (5, 1, 6) and weights.shape == (5, 1, 9) and not weights.requires_grad


def test_refusals_through_python():
    from ggrt_official_amd import epipolar_encoded_attention_core, fused_epipolar_encoded_attention
    case = make_enc_case(5, 9, 6, 7, 1, 6, 3, 31, project_out=False)
    x, f, d, w_enc, b_enc, w_q, w_kv = [case[k].to(device=DEV, dtype=torch.float32) for k in ENC_LEAVES[:7]]
    with pytest.raises(ValueError, match="ONE query token per ray"):
        fused_epipolar_encoded_attention(x.expand(5, 2, 6), f, d, w_enc, b_enc, w_q, w_kv, None, None, 1)
    with pytest.raises(RuntimeError, match="outside 1..64"):
        fused_epipolar_encoded_attention(x, f.repeat(1, 8, 1), d.repeat(1, 8), w_enc, b_enc, w_q, w_kv, None, None, 1)      # 72 samples
    with pytest.raises(ValueError, match="depth"):
        fused_epipolar_encoded_attention(x, f, d[:, :8], w_enc, b_enc, w_q, w_kv, None, None, 1)
    with pytest.raises(ValueError, match="depth"):
        epipolar_encoded_attention_core(torch.zeros(5, 1, 7, device=DEV), torch.zeros(5, 1, 6, device=DEV), f, d.t().contiguous())
    with pytest.raises(ValueError, match="odd"):
        epipolar_encoded_attention_core(torch.zeros(5, 1, 7, device=DEV), torch.zeros(5, 1, 5, device=DEV), f, d)
    with pytest.raises(ValueError, match="2\\*num_octaves"):
        fused_epipolar_encoded_attention(x, f, d, w_enc[:, :5], b_enc, w_q, w_kv, None, None, 1)
    with pytest.raises(RuntimeError, match="num_octaves 17 is outside 1..16"):
        epipolar_encoded_attention_core(torch.zeros(5, 1, 7, device=DEV), torch.zeros(5, 1, 34, device=DEV), f, d)
    with pytest.raises(RuntimeError, match="num_octaves 17 is outside 1..16"):
        fused_epipolar_encoded_attention(x, f, d, torch.zeros(7, 34, device=DEV), b_enc, w_q, w_kv, None, None, 1)


def test_the_encoding_alone_is_within_1e_6_of_the_contract():
    """qk = 0, qe = 0 and S = 1: the one weight is 1 and ctx_e[n,h,:] is pe(d_n) as the kernel evaluates it.  Against the contract
    (the reference's module on its float32 constants, in float64, at the float32 depth the kernel reads): the reduced argument is
    below 8, so its rounding is below 4.8e-7, plus one sine rounding — 1e-6 absolute.  The reference's own float32 module is at
    1.3e-4 at octave 10; printed next to the kernel's figure for the record."""
    from ggrt_official_amd import epipolar_encoded_attention_core
    o, h = 16, 2
    special = torch.tensor([0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 ** -20, -0.25, 1.5], dtype=torch.float32)
    d = torch.cat([special, torch.rand(64, generator=torch.Generator().manual_seed(61), dtype=torch.float32)])
    n = d.numel()
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    ctx_f, ctx_e, attn = epipolar_encoded_attention_core(zeros(n, h, 1), zeros(n, h, 2 * o), zeros(n, 1, 1), d.to(DEV).reshape(n, 1))
    assert ctx_e.shape == (n, h, 2 * o) and bool((attn == 1).all()) and bool((ctx_f == 0).all())
    want = positional_encoding(d.double(), o)
    err = (ctx_e.double().cpu() - want[:, None, :]).abs()
    module32 = (positional_encoding(d, o).double() - want).abs()
    for k in range(o):
        print(f"octave {k:2d}: kernel {float(err[..., 2 * k:2 * k + 2].max()):.3e}   float32 module {float(module32[:, 2 * k:2 * k + 2].max()):.3e}")
    assert torch.equal(ctx_e[:, 0], ctx_e[:, 1])
    assert float(err.max()) <= 1e-6, float(err.max())


def _core_inputs(n, s, c, h, o, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    depth = torch.rand((n, s), generator=gen, dtype=torch.float32).double()
    return dict(qk=r(n, h, c), qe=r(n, h, 2 * o), f=r(n, s, c), d=depth, g_f=r(n, h, c), g_e=r(n, h, 2 * o))


def _run_core(t, depth_grad=True):
    from ggrt_official_amd import epipolar_encoded_attention_core
    leaves = [t[k].to(device=DEV, dtype=torch.float32).requires_grad_(depth_grad or k != "d") for k in ("qk", "qe", "f", "d")]
    ctx_f, ctx_e, attn = epipolar_encoded_attention_core(*leaves)
    grads = torch.autograd.grad([ctx_f, ctx_e], [l for l in leaves if l.requires_grad],
                                [t["g_f"].to(device=DEV, dtype=torch.float32), t["g_e"].to(device=DEV, dtype=torch.float32)])
    return (ctx_f.detach(), ctx_e.detach(), attn) + tuple(grads)


CORE_NAMES = ("ctx_f", "ctx_e", "attn", "g_qk", "g_qe", "g_f", "g_d")


@pytest.mark.parametrize("s", [1, 3, 32, 33, 64])
def test_rows_of_attn_and_the_bias_of_the_encoding(s):
    """The weights are a softmax over the samples; with qk = 0 and qe = 0 each is 1/S rounded once.  b_enc never reaches the
    kernel (qk·b is the same for every sample): a constant added to it leaves attn bit-equal, and moves the output by what it
    moves the literal route's — compared as differences of outputs, each of which the bar above holds to max(4·e_torch32, 1e-6) of
    the largest output, so the difference of two is held to twice that."""
    from ggrt_official_amd import epipolar_encoded_attention_core, fused_epipolar_encoded_attention
    n, c, h, o = 5, 20, 3, 3
    t = _core_inputs(n, s, c, h, o, 40 + s)
    f32 = lambda x: x.to(device=DEV, dtype=torch.float32)
    ctx_f, ctx_e, attn = epipolar_encoded_attention_core(f32(t["qk"]) * 3, f32(t["qe"]) * 3, f32(t["f"]), f32(t["d"]))
    assert attn.shape == (n, h, s) and not attn.requires_grad and bool((attn >= 0).all())
    assert float((attn.double().sum(-1) - 1).abs().max()) <= 1e-6
    _, _, attn0 = epipolar_encoded_attention_core(torch.zeros_like(f32(t["qk"])), torch.zeros_like(f32(t["qe"])), f32(t["f"]), f32(t["d"]))
    exact = torch.tensor(1.0 / s, dtype=torch.float64)
    assert float((attn0.double() - exact).abs().max()) <= 2.0 ** -24 * float(exact)

    case = make_enc_case(n, s, 6, c, h, 2, o, 140 + s)
    moved = dict(case, b_enc=case["b_enc"] + 0.75)
    names = ENC_LEAVES
    outs = {}
    for tag, cs in (("base", case), ("moved", moved)):
        with torch.no_grad():
            a64 = [cs[k] for k in names]
            a32 = [cs[k].to(device=DEV, dtype=torch.float32) for k in names]
            outs[tag] = (encoded_literal(*a64, h), encoded_literal(*a32, h).double().cpu(),
                         *[v.double().cpu() for v in fused_epipolar_encoded_attention(*a32, h, return_weights=True)])
    assert torch.equal(outs["base"][3], outs["moved"][3])                # attn: to the bit
    d_ref, d_t32, d_ker = (outs["moved"][i] - outs["base"][i] for i in range(3))
    assert float(d_ref.abs().max()) > 0
    scale = max(float(outs[tag][0].abs().max()) for tag in outs)
    e_t32 = max(float((outs[tag][1] - outs[tag][0]).abs().max()) for tag in outs) / scale
    e_ker = float((d_ker - d_ref).abs().max()) / scale
    print(f"S={s}: the move of the output: e_kernel {e_ker:.3e}, e_torch32 of one output {e_t32:.3e}, of its move {float((d_t32 - d_ref).abs().max()) / scale:.3e}")
    assert e_ker <= 2 * max(4 * e_t32, 1e-6)


def test_the_core_matches_its_float64_formulas():
    """the kernels alone, without the projections around them: all seven outputs against enc_core_forward / enc_core_backward at
    the float32 inputs' own values.  The bar is the one the plain core's test derives for a 68-term float32 dot product (2e-4); the
    encoding adds 20 terms of size <= 0.3 to a logit.  g_d carries the factor F·2^k (3 200 at octave 10) and is normalised by its
    own largest reference value, as the others are."""
    t = _core_inputs(7, 33, 68, 5, 10, 51)
    t["qk"], t["qe"] = t["qk"] * 0.3, t["qe"] * 0.3
    t = {k: v.float().double() for k, v in t.items()}
    ctx_f64, ctx_e64, attn64 = enc_core_forward(t["qk"], t["qe"], t["f"], t["d"])
    want = (ctx_f64, ctx_e64, attn64) + enc_core_backward(t["qk"], t["qe"], t["f"], t["d"], attn64, t["g_f"], t["g_e"])
    got = _run_core(t)
    for name, g, w in zip(CORE_NAMES, got, want):
        assert g.shape == w.shape, name
        e = _err(g.double().cpu(), w)
        print(f"core {name:6s} e {e:.3e}")
        assert e <= 2e-4, (name, e)


def test_with_a_zero_qe_the_core_agrees_with_the_plain_core():
    from ggrt_official_amd import epipolar_attention_core
    t = _core_inputs(9, 33, 68, 5, 10, 57)
    t["qe"] = torch.zeros_like(t["qe"])
    t["g_e"] = torch.zeros_like(t["g_e"])
    got = dict(zip(CORE_NAMES, _run_core(t)))
    qk = t["qk"].to(device=DEV, dtype=torch.float32).requires_grad_(True)
    z = t["f"].to(device=DEV, dtype=torch.float32).requires_grad_(True)
    ctx, attn = epipolar_attention_core(qk, z)
    g_qk, g_z = torch.autograd.grad(ctx, [qk, z], t["g_f"].to(device=DEV, dtype=torch.float32))
    for name, a, b in (("ctx_f", got["ctx_f"], ctx.detach()), ("attn", got["attn"], attn), ("g_qk", got["g_qk"], g_qk), ("g_f", got["g_f"], g_z)):
        e = _err(a.double(), b.double())
        print(f"{name:6s} against the plain core: {e:.3e}")
        assert e <= 1e-6, (name, e)


def test_forward_and_backward_give_the_same_bits_twice_and_depth_gradient_is_optional():
    t = _core_inputs(257, 32, 128, 4, 10, 52)
    runs = [_run_core(t) for _ in range(2)]
    assert len(runs[0]) == 7 and all(float(x.abs().max()) > 0 for x in runs[0])
    for a, b, name in zip(runs[0], runs[1], CORE_NAMES):
        assert torch.equal(a, b), name
    without = _run_core(t, depth_grad=False)          # dL_ddepth = NULL: the other six are the same bits
    assert len(without) == 6
    for a, b, name in zip(runs[0][:6], without, CORE_NAMES):
        assert torch.equal(a, b), name


def test_memory_stays_below_twice_the_bytes_of_features():
    """Derived as for the plain route: g_f is 1 × the bytes of features; the [N,H,C]- and [N,H·D]-sized tensors are the ones the
    plain route has (1/8 of features each at this shape; it measured 1.77 ×); the [N,H,E] and [N,S] tensors add under 0.03 ×.  So
    the rise of the peak over a forward + backward, above what is allocated once the inputs exist, is at most 2 × the bytes of
    features.  The parent's route — the encoding in torch, then `fused_epipolar_attention` on z — holds z, the [N,S,E] encoding and
    g_z on top of its own 1.77 × and cannot meet that bound: asserted, so that the test shows what the fold buys."""
    from ggrt_official_amd import fused_epipolar_attention, fused_epipolar_encoded_attention
    n, s, c, h, d, dim, o = 1024, 32, 128, 4, 128, 128, 10
    case = make_enc_case(n, s, dim, c, h, d, o, 53)

    def parent(x, features, depth, w_enc, b_enc, *rest):
        z = features + torch.nn.functional.linear(positional_encoding(depth, o), w_enc, b_enc)
        return fused_epipolar_attention(x, z, *rest)

    def step(fn, rays):
        leaf = [case[k][:rays].clone() if k in ("x", "features", "depth") else case[k].clone() for k in ENC_LEAVES]
        leaf = [t.to(device=DEV, dtype=torch.float32).requires_grad_(True) for t in leaf]
        g = case["g_out"][:rays].to(device=DEV, dtype=torch.float32)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn(*leaf, h)
        out.backward(g)
        torch.cuda.synchronize()
        assert all(t.grad is not None and t.grad.shape == t.shape for t in leaf)
        return torch.cuda.max_memory_allocated() - before, leaf[1].numel() * 4

    rises = {}
    for name, fn in (("encoded", fused_epipolar_encoded_attention), ("parent", parent)):
        step(fn, 8)      # (the BLAS library's workspace and the code objects exist from here on)
        rises[name], f_bytes = step(fn, n)
        print(f"{name}: rise of the peak {rises[name] / 2 ** 20:.2f} MiB, features {f_bytes / 2 ** 20:.2f} MiB, ratio {rises[name] / f_bytes:.3f}")
    assert f_bytes == n * s * c * 4 and rises["encoded"] <= 2 * f_bytes, (rises, f_bytes)
    assert rises["parent"] > 2 * f_bytes, (rises, f_bytes)


def test_element_offsets_past_two_to_the_31():
    """N·S·C = 2^31 + 8·2^14 floats: the last rays lie past a 32-bit element offset.  They must equal, to the bit, the same rays
    computed on their own (N = 8), forward and backward."""
    from ggrt_official_amd import epipolar_encoded_attention_core
    s, c, h, o = 64, 256, 1, 1
    n = (1 << 31) // (s * c) + 8
    rnd = lambda shape, seed: torch.empty(shape, dtype=torch.float32, device=DEV).normal_(generator=torch.Generator(DEV).manual_seed(seed))
    f, qk, qe = rnd((n, s, c), 54), rnd((n, h, c), 55) * 0.2, rnd((n, h, 2 * o), 58)
    d = torch.empty((n, s), dtype=torch.float32, device=DEV).uniform_(generator=torch.Generator(DEV).manual_seed(59))
    g_f, g_e = rnd((n, h, c), 56), rnd((n, h, 2 * o), 60)

    def run(inputs, grads):
        leaves = [t.requires_grad_(True) for t in inputs]
        ctx_f, ctx_e, attn = epipolar_encoded_attention_core(*leaves)
        return (ctx_f.detach(), ctx_e.detach(), attn) + torch.autograd.grad([ctx_f, ctx_e], leaves, grads)

    tail = run([t[-8:].clone() for t in (qk, qe, f, d)], [g_f[-8:].clone(), g_e[-8:].clone()])
    whole = [t[-8:] for t in run([qk, qe, f, d], [g_f, g_e])]
    assert all(float(t.abs().max()) > 0 for t in tail)
    for a, b, name in zip(whole, tail, CORE_NAMES):
        assert torch.equal(a, b), name
