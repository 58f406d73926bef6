"""`FusedSepConvGRU` / `FusedConvGRU`, `fused_gru_half`, `gru_gate` and `gru_blend` (csrc/gru_gates.hip) on the GPU against the torch
restatement of GGRt's `SepConvGRU` / `ConvGRU` (tests/gru_reference.py, pinned to the reference's own modules by the fixtures).

Three routes: `ref` the literal restatement in float64 on the CPU, `t32` the literal restatement in float32 on the device, `ker` the
modules over the kernels.  Buffers the launches must write whole are filled with NaN first.  The bar, every figure printed before it
is asserted, for h' and each gradient (h, x, the six parameters of every half): max |ker - ref| / max |ref| <= max(4 x the same
figure of t32, 1e-6).  The references of a shape are computed once and shared.

Bit-equality is asserted on the kernels' own entry points (`gru_gate`, `gru_blend`); what passes through MIOpen's convolutions is
held to the bar, since a convolution's backward need not sum in one order on every call."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import ggrt_official_amd.splatting as splatting
from ggrt_official_amd import FusedConvGRU, FusedSepConvGRU, fused_gru_half, gru_blend, gru_gate
from tests.gru_reference import (HALVES, blend_backward, blend_forward, gate_backward, gate_forward, literal_gru, make_gru_case, result_keys, run_gru,
                                 split_params)
from tests.test_gru_reference import GPU_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODULES = {"sep": FusedSepConvGRU, "conv": FusedConvGRU}


@pytest.fixture(autouse=True)
def _poison():
    splatting._IMAGE_LOSS_POISON = True
    yield
    splatting._IMAGE_LOSS_POISON = False


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a.reshape(b.shape) - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _bar(name, k, ker, ref, t32):
    assert ker is not None and ker.dtype == torch.float32 and not torch.isnan(ker).any(), (name, k)
    assert tuple(ker.shape) == tuple(ref.shape), (name, k, ker.shape, ref.shape)
    e32, e = _rel(t32, ref), _rel(ker, ref)
    print(f"{name} {k}: kernel {e:.3e}, t32 {e32:.3e}")
    assert e <= max(4 * e32, 1e-6), (name, k, e, e32)


@functools.lru_cache(maxsize=None)
def _references(kind, shape):
    N, ch, cx, H, W, seed = GPU_SHAPES[shape]
    case = make_gru_case(kind, N, ch, cx, H, W, seed)
    return case, run_gru("literal", kind, case, torch.float64, "cpu"), run_gru("literal", kind, case, torch.float32, DEV)


@pytest.mark.parametrize("shape", list(GPU_SHAPES))
@pytest.mark.parametrize("kind", sorted(MODULES))
def test_modules_against_the_float64_literal_restatement(kind, shape):
    """On an MI355X every case meets the bar except two figures at 1x128x48x63, both the weight gradient of the merged h-side z/r
    convolution, which MIOpen forms: conv dL/dw_zr_h 1.131e-06 (t32 1.80e-07, bar 1e-06) and sep dL/dw_zr_h2 1.025e-06 (t32
    1.87e-07, bar 1e-06); every other figure of those two cases, and all of 5x128x48x63, is within it.  MIOpen's weight gradient
    alone at that problem ([256,128,kh,kw] from one 48 x 63 map), fed the float64 route's h and dL/da_zr rounded to float32, is
    1.0e-06 (3x3) and 1.2e-06 (1x5) from float64 — float32 torch on the CPU has 1.6e-06 and 9.7e-07 there — where the literal
    route's [128,288,kh,kw] problems gave 1.1e-06 and 2.4e-07 in one process and 1.8e-07 in another: a 3024-term float32 sum whose
    error depends on the algorithm MIOpen picks, not on the gate kernels, whose own outputs (dL/da_zr, dL/dh, dL/dx) are within the
    bar.  The bar stays as set; these two cases fail on that figure."""
    case, ref, t32 = _references(kind, shape)
    ker = run_gru(MODULES[kind], kind, case, torch.float32, DEV)
    for k in result_keys(kind):
        _bar(f"{kind} {shape}", k, ker[k], ref[k], t32[k])


@pytest.mark.parametrize("need", [c for n in range(4) for c in itertools.combinations(("h", "x", "params"), n)], ids=lambda c: "+".join(c) or "nothing")
@pytest.mark.parametrize("kind", sorted(MODULES))
def test_every_subset_of_requires_grad(kind, need):
    """A gradient's value does not depend on which others are asked for: the full references serve every subset."""
    case, ref, t32 = _references(kind, "3x5x9x23")
    ker = run_gru(MODULES[kind], kind, case, torch.float32, DEV, need=need)
    _bar(kind, "out", ker["out"], ref["out"], t32["out"])
    for k in result_keys(kind)[1:]:
        wanted = (k in ("g_h", "g_x") and k[2:] in need) or (k not in ("g_h", "g_x") and "params" in need)
        if wanted:
            _bar(f"{kind} need={need}", k, ker[k], ref[k], t32[k])
        else:
            assert ker[k] is None, (need, k)


def _gate_inputs(N, ch, H, W, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    t = dict(a_zr_h=2 * rnd(N, 2 * ch, H, W), a_zr_x=2 * rnd(N, 2 * ch, H, W), h=torch.tanh(rnd(N, ch, H, W)), a_q_h=1.5 * rnd(N, ch, H, W),
             a_q_x=1.5 * rnd(N, ch, H, W), z=torch.sigmoid(2 * rnd(N, ch, H, W)), g=rnd(N, ch, H, W), g2=rnd(N, ch, H, W))
    return {k: v.to(dtype) for k, v in t.items()}


def _leaves(t, names, dtype, device):
    out = {k: v.to(device=device, dtype=dtype).clone() for k, v in t.items()}
    for k in names:
        out[k].requires_grad_(True)
    return out


ALONE_SHAPES = [(1, 3, 3, 5), (2, 3, 3, 5), (2, 4, 5, 7), (3, 5, 9, 23)]


@pytest.mark.parametrize("both", [True, False], ids=["two_addends", "one_addend"])
@pytest.mark.parametrize("dims", ALONE_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_gate_alone_against_its_float64_formulas(dims, both):
    """rh only carries a gradient here (z's slot belongs to gru_blend): dL/da_zr has an exactly zero z half and the r half of the
    formula; dL/dh = dL/drh r."""
    t = _gate_inputs(*dims, seed=1040)
    ch, names = dims[1], ("a_zr_h", "a_zr_x", "h") if both else ("a_zr_h", "h")

    def torch_route(dtype, device):
        v = _leaves(t, names, dtype, device)
        z, r, rh = gate_forward(v["a_zr_h"], v["a_zr_x"] if both else None, v["h"])
        (rh * v["g"]).sum().backward()
        return dict(z=z.detach(), rh=rh.detach(), **{"g_" + k: v[k].grad for k in names}), r.detach()

    (ref, r64), (t32, _) = torch_route(torch.float64, "cpu"), torch_route(torch.float32, DEV)
    v = _leaves(t, names, torch.float32, DEV)
    z, rh = gru_gate(v["a_zr_h"], v["a_zr_x"] if both else None, v["h"])
    (rh * v["g"]).sum().backward()
    ker = dict(z=z.detach(), rh=rh.detach(), **{"g_" + k: v[k].grad for k in names})
    for k in ref:
        _bar(f"gate {dims}", k, ker[k], ref[k], t32[k])
    assert bool((ker["g_a_zr_h"][:, :ch] == 0).all())
    g_a_r, g_h = gate_backward(t["g"], t["h"], r64)
    assert _rel(ker["g_a_zr_h"][:, ch:], g_a_r) <= 1e-5 and _rel(ker["g_h"], g_h) <= 1e-5
    if both:
        assert torch.equal(ker["g_a_zr_h"], ker["g_a_zr_x"])


@pytest.mark.parametrize("both", [True, False], ids=["two_addends", "one_addend"])
@pytest.mark.parametrize("dims", ALONE_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_blend_alone_against_its_float64_formulas(dims, both):
    t = _gate_inputs(*dims, seed=1041)
    names = ("a_q_h", "a_q_x", "h") if both else ("a_q_h", "h")

    def torch_route(dtype, device):
        v = _leaves(t, names, dtype, device)
        q, out = blend_forward(v["a_q_h"], v["a_q_x"] if both else None, v["z"], v["h"])
        (out * v["g"]).sum().backward()
        return dict(out=out.detach(), **{"g_" + k: v[k].grad for k in names}), q.detach()

    (ref, q64), (t32, _) = torch_route(torch.float64, "cpu"), torch_route(torch.float32, DEV)
    v = _leaves(t, names, torch.float32, DEV)
    out = gru_blend(v["a_q_h"], v["a_q_x"] if both else None, v["z"], v["h"])
    assert out.data_ptr() != v["h"].data_ptr()
    (out * v["g"]).sum().backward()
    ker = dict(out=out.detach(), **{"g_" + k: v[k].grad for k in names})
    for k in ref:
        _bar(f"blend {dims}", k, ker[k], ref[k], t32[k])
    g_a_q, _, g_h = blend_backward(t["g"], t["z"], q64, t["h"])
    assert _rel(ker["g_a_q_h"], g_a_q) <= 1e-5 and _rel(ker["g_h"], g_h) <= 1e-5
    if both:
        assert torch.equal(ker["g_a_q_h"], ker["g_a_q_x"])


def _chain(v, w=0.75):
    """gate -> a stand-in for the w_q_h convolution -> blend, plus a second consumer of rh; returns what a training step sees"""
    z, rh = gru_gate(v["a_zr_h"], v["a_zr_x"], v["h"])
    out = gru_blend(v["a_q_h"] + w * rh, v["a_q_x"], z, v["h"])
    return z, rh, out


def _chain_step(v, names):
    z, rh, out = _chain(v)
    grads = torch.autograd.grad((out * v["g"]).sum() + (rh * v["g2"]).sum(), [v[k] for k in names])
    return dict(z=z.detach(), rh=rh.detach(), out=out.detach(), **{"g_" + k: g for k, g in zip(names, grads)})


CHAIN_LEAVES = ("a_zr_h", "a_zr_x", "h", "a_q_h", "a_q_x")


@pytest.mark.parametrize("dims", [(2, 3, 3, 5), (3, 5, 9, 23), (2, 4, 5, 7)], ids=lambda d: "x".join(map(str, d)))
def test_the_chained_kernels_against_float64_and_two_runs_give_the_same_bits(dims):
    t = _gate_inputs(*dims, seed=1042)
    ch = dims[1]

    def torch_route(dtype, device):
        v = _leaves(t, CHAIN_LEAVES, dtype, device)
        z, r, rh = gate_forward(v["a_zr_h"], v["a_zr_x"], v["h"])
        q, out = blend_forward(v["a_q_h"] + 0.75 * rh, v["a_q_x"], z, v["h"])
        grads = torch.autograd.grad((out * v["g"]).sum() + (rh * v["g2"]).sum(), [v[k] for k in CHAIN_LEAVES])
        return dict(z=z.detach(), rh=rh.detach(), out=out.detach(), **{"g_" + k: g for k, g in zip(CHAIN_LEAVES, grads)})

    ref, t32 = torch_route(torch.float64, "cpu"), torch_route(torch.float32, DEV)
    ker = _chain_step(_leaves(t, CHAIN_LEAVES, torch.float32, DEV), CHAIN_LEAVES)
    for k in ref:
        _bar(f"chain {dims}", k, ker[k], ref[k], t32[k])
    assert float(ker["g_a_zr_h"][:, :ch].abs().max()) > 0 and float(ker["g_a_zr_h"][:, ch:].abs().max()) > 0
    again = _chain_step(_leaves(t, CHAIN_LEAVES, torch.float32, DEV), CHAIN_LEAVES)
    for k in ker:
        assert torch.equal(ker[k], again[k]), k


@pytest.mark.parametrize("dims", [(2, 3, 3, 5), (2, 4, 5, 7)], ids=["scalar_path", "vector_path"])
def test_preactivations_of_exactly_100_saturate_exactly(dims):
    N, ch, H, W = dims
    gen = torch.Generator().manual_seed(1043)
    sign = lambda *s: (torch.randint(0, 2, s, generator=gen).float() * 2 - 1) * 100.0
    a_zr = sign(N, 2 * ch, H, W).to(DEV).requires_grad_(True)
    a_q = sign(N, ch, H, W).to(DEV).requires_grad_(True)
    h = torch.tanh(torch.randn(N, ch, H, W, generator=gen)).to(DEV).requires_grad_(True)
    g, g2 = torch.randn(N, ch, H, W, generator=gen).to(DEV), torch.randn(N, ch, H, W, generator=gen).to(DEV)
    z, rh = gru_gate(a_zr, None, h)
    out = gru_blend(a_q, None, z, h)
    g_a_zr, g_a_q, g_h = torch.autograd.grad((out * g).sum() + (rh * g2).sum(), (a_zr, a_q, h))
    zd, hd = z.detach(), h.detach()
    want_z, want_r, want_q = (a_zr.detach()[:, :ch] > 0).float(), (a_zr.detach()[:, ch:] > 0).float(), torch.sign(a_q.detach())
    assert torch.equal(zd, want_z) and 0 < float(want_z.mean()) < 1          # z exactly 0 or 1, both present
    assert torch.equal(rh.detach(), want_r * hd) and 0 < float(want_r.mean()) < 1          # r exactly 0 or 1
    assert torch.equal(out.detach(), torch.where(want_z == 1, want_q, hd))          # h' exactly q = +-1, or exactly h
    assert bool((g_a_zr == 0).all()) and bool((g_a_q == 0).all())          # dL/da_z, dL/da_r, dL/da_q exactly 0.0
    for t in (zd, rh, out, g_a_zr, g_a_q, g_h):
        assert not torch.isnan(t).any() and not torch.isinf(t).any()
    assert torch.equal(g_h, g * (1 - want_z) + g2 * want_r)
    # ... and the largest finite pre-activations stay finite
    big = torch.tensor([3.0e38, -3.0e38, 88.0, -88.0, 104.0, -104.0, 0.0, -0.0] * 2, device=DEV).reshape(1, 4, 2, 2)
    zb, rhb = gru_gate(big, None, torch.ones(1, 2, 2, 2, device=DEV))
    ob = gru_blend(big[:, :2], None, zb, torch.ones(1, 2, 2, 2, device=DEV))
    assert bool(torch.isfinite(zb).all()) and bool(torch.isfinite(rhb).all()) and bool(torch.isfinite(ob).all())
    assert float(zb.min()) == 0.0 and float(zb.max()) == 1.0


def test_z_is_differentiable_through_one_blend_only():
    t = _gate_inputs(1, 2, 3, 4, seed=1044)
    v = _leaves(t, CHAIN_LEAVES, torch.float32, DEV)
    z, rh, out = _chain(v)
    with pytest.raises(RuntimeError, match="z is differentiable through one gru_blend only"):
        (out.sum() + z.sum()).backward()


def test_a_strided_h_and_x():
    kind, shape = "sep", "3x5x9x23"
    case, ref, t32 = _references(kind, shape)
    strided = dict(case, h=case["h"].transpose(2, 3).contiguous().transpose(2, 3), x=case["x"].transpose(1, 3).contiguous().transpose(1, 3))
    assert not strided["h"].is_contiguous() and not strided["x"].is_contiguous()

    def route(ch, cx):
        m = FusedSepConvGRU(ch, cx)
        fwd = m.forward
        m.forward = lambda h, x: fwd(h.transpose(2, 3).contiguous().transpose(2, 3), x.transpose(1, 3).contiguous().transpose(1, 3))
        return m

    ker = run_gru(route, kind, case, torch.float32, DEV)
    for k in result_keys(kind):
        _bar("strided", k, ker[k], ref[k], t32[k])


def _busy(a):
    for _ in range(8):
        a = (a @ a).clamp(-1, 1)
    return a


def test_on_a_side_stream_with_a_busy_default_stream():
    kind, shape = "sep", "3x5x9x23"
    case, ref, t32 = _references(kind, shape)
    t = _gate_inputs(3, 5, 9, 23, seed=1045)
    plain = _chain_step(_leaves(t, CHAIN_LEAVES, torch.float32, DEV), CHAIN_LEAVES)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    v = _leaves(t, CHAIN_LEAVES, torch.float32, DEV)
    torch.cuda.synchronize()
    a = _busy(a)            # the default stream is busy while the side stream works
    with torch.cuda.stream(side):
        got = _chain_step(v, CHAIN_LEAVES)
        ker = run_gru(MODULES[kind], kind, case, torch.float32, DEV)
    a = _busy(a)
    side.synchronize()
    torch.cuda.synchronize()
    for k in plain:
        assert not torch.isnan(got[k]).any() and torch.equal(got[k], plain[k]), k
    for k in result_keys(kind):
        _bar("side stream", k, ker[k], ref[k], t32[k])


def test_graph_replay_with_two_refreshes_equals_eager():
    """Forward + backward of the chained kernels captured once; replayed with the second inputs, then with the first again, the
    outputs NaN before each."""
    dims = (2, 4, 5, 7)
    first, second = _gate_inputs(*dims, seed=1046), _gate_inputs(*dims, seed=1047)
    eager = {id(c): _chain_step(_leaves(c, CHAIN_LEAVES, torch.float32, DEV), CHAIN_LEAVES) for c in (first, second)}
    assert not torch.equal(eager[id(first)]["out"], eager[id(second)]["out"])
    v = _leaves(first, CHAIN_LEAVES, torch.float32, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # (warm-up on a side stream, as torch's graph recipe asks)
        for _ in range(2):
            _chain_step(v, CHAIN_LEAVES)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _chain_step(v, CHAIN_LEAVES)
    for case in (second, first):
        with torch.no_grad():
            for k, dst in v.items():
                dst.copy_(case[k].to(device=DEV, dtype=torch.float32))
            for buf in got.values():
                buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in got:
            assert not torch.isnan(got[k]).any() and torch.equal(got[k], eager[id(case)][k]), k


def test_every_refusal():
    route = "SepConvGRU.forward / ConvGRU.forward"
    ch, cx = 3, 2
    mk = lambda N=2, H=4, W=5: (torch.zeros(N, ch, H, W, device=DEV), torch.zeros(N, cx, H, W, device=DEV))
    w = lambda: [torch.zeros(2 * ch, ch, 1, 5, device=DEV), torch.zeros(2 * ch, cx, 1, 5, device=DEV), torch.zeros(2 * ch, device=DEV),
                 torch.zeros(ch, ch, 1, 5, device=DEV), torch.zeros(ch, cx, 1, 5, device=DEV), torch.zeros(ch, device=DEV)]
    names = ("h", "x", "w_zr_h", "w_zr_x", "b_zr", "w_q_h", "w_q_x", "b_q")
    for i, name in enumerate(names):
        a = list(mk()) + w()
        a[i] = a[i].double()
        with pytest.raises(ValueError, match=name + " is torch.float64.*" + route):
            fused_gru_half(*a, (0, 2))
        a = list(mk()) + w()
        a[i] = a[i].cpu()
        with pytest.raises(ValueError, match=name + " is on cpu.*" + route):
            fused_gru_half(*a, (0, 2))
    if torch.cuda.device_count() > 1:
        a = list(mk()) + w()
        a[1] = a[1].to("cuda:1")
        with pytest.raises(ValueError, match="x is on cuda:1.*not on one device.*" + route):
            fused_gru_half(*a, (0, 2))
    h, x = mk()
    with pytest.raises(ValueError, match="x .* does not have h's batch and spatial sizes.*" + route):
        fused_gru_half(h, x[:1], *w(), (0, 2))
    with pytest.raises(ValueError, match="x .* does not have h's batch and spatial sizes.*" + route):
        fused_gru_half(h, x[..., :4], *w(), (0, 2))
    with pytest.raises(ValueError, match="are not \\[N, Ch, H, W\\].*" + route):
        fused_gru_half(h[0], x[0], *w(), (0, 2))
    with pytest.raises(ValueError, match="is empty.*" + route):
        fused_gru_half(h[:0], x[:0], *w(), (0, 2))
    for i, name in enumerate(names[2:]):
        a = w()
        a[i] = a[i][:-1]
        with pytest.raises(ValueError, match=name + " .* is not .*Ch = 3, Cx = 2.*" + route):
            fused_gru_half(h, x, *a, (0, 2))
    with pytest.raises(ValueError, match="w_zr_h .* is not .*" + route):          # a 1 x 5 kernel with a 5 x 1 padding
        fused_gru_half(h, x, *w(), (2, 0))
    with pytest.raises(ValueError, match="padding.*" + route):
        fused_gru_half(h, x, *w(), 2)
    with pytest.raises(ValueError, match="x .* has|w_zr_x .* is not"):          # a module built for another input_dim
        FusedSepConvGRU(ch, cx + 1).to(DEV)(h, x)
    with pytest.raises(ValueError, match="a_zr_h .* has 3 channels, not 6.*" + route):
        gru_gate(h, None, h)
    with pytest.raises(ValueError, match="z .* does not have h's batch and spatial sizes.*" + route):
        gru_blend(h, None, h[:1], h)
    with pytest.raises(ValueError, match="h .* is empty.*" + route):
        gru_gate(torch.zeros(0, 6, 4, 5, device=DEV), None, h[:0])
    assert fused_gru_half(h, x, *w(), (0, 2)).shape == h.shape and FusedConvGRU(ch, cx).to(DEV)(h, x).shape == h.shape


class _UpdateLoop(torch.nn.Module):
    """encoder -> GRU -> head, four steps, shaped as BasicUpdateBlockDepth (ggrt/optimizer.py:145-174) with hidden 8"""

    def __init__(self, gru, hidden=8, context=4):
        super().__init__()
        self.encoder = torch.nn.Conv2d(1, hidden, 3, padding=1)
        self.head = torch.nn.Conv2d(hidden, 1, 3, padding=1)
        self.gru = gru

    def forward(self, net, inv_depth, context):
        outs = []
        for _ in range(4):
            inp = torch.cat([context, F.relu(self.encoder(inv_depth))], dim=1)
            net = self.gru(net, inp)
            inv_depth = inv_depth + torch.tanh(self.head(net))
            outs.append(inv_depth)
        return net, outs


class _LiteralGRU(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.p = torch.nn.ParameterDict({k.replace(".", "__"): torch.nn.Parameter(v.clone()) for k, v in sd.items()})

    def forward(self, h, x):
        return literal_gru("sep", {k.replace("__", "."): v for k, v in self.p.items()}, h, x)


def test_call_site_four_steps_of_an_update_block():
    hidden, context, N, H, W = 8, 4, 2, 6, 9
    gen = torch.Generator().manual_seed(1050)
    case = make_gru_case("sep", N, hidden, hidden + context, H, W, 1051)
    net0, ctx, d0 = case["h"], case["x"][:, :context], torch.rand(N, 1, H, W, generator=gen, dtype=torch.float64)
    g = torch.randn(4, N, 1, H, W, generator=gen, dtype=torch.float64)
    torch.manual_seed(1052)
    outer = {k: v.double() for k, v in _UpdateLoop(torch.nn.Identity()).state_dict().items()}

    def run(fused, dtype, device):
        if fused:
            gru = FusedSepConvGRU(hidden, hidden + context)
            gru.load_reference_state_dict({k: v.float() for k, v in case["sd"].items()})
        else:
            gru = _LiteralGRU(case["sd"])
        loop = _UpdateLoop(gru).to(device=device, dtype=dtype)
        loop.load_state_dict({k: v.to(dtype) for k, v in outer.items()}, strict=False)
        net_in = net0.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
        net, outs = loop(net_in, d0.to(device=device, dtype=dtype), ctx.to(device=device, dtype=dtype))
        (sum((o * gg).sum() for o, gg in zip(outs, g.to(device=device, dtype=dtype))) + net.sum()).backward()
        res = dict(net=net.detach(), last=outs[-1].detach(), g_net=net_in.grad, **{"g_" + k: v.grad for k, v in loop.named_parameters() if not k.startswith("gru.")})
        params = dict(gru.named_parameters())
        if fused:
            res.update({"g_" + k: v.grad for k, v in params.items()})
        else:
            res.update({"g_" + k: v for k, v in split_params("sep", {k.replace("__", ".")[2:]: v.grad for k, v in params.items()}, hidden).items()})
        return res

    ref, t32, ker = run(False, torch.float64, "cpu"), run(False, torch.float32, DEV), run(True, torch.float32, DEV)
    assert {"g_encoder.weight", "g_encoder.bias", "g_head.weight", "g_head.bias"} <= set(ker) and len(ker) == 3 + 4 + 12
    for k in ref:
        _bar("call site", k, ker[k], ref[k], t32[k])
        assert float(ker[k].abs().max()) > 0, k
