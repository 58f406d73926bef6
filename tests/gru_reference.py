"""Torch restatements of GGRt's GRUs (ggrt/optimizer.py: `ConvGRU.forward` lines 40-48, `SepConvGRU.forward` lines 63-78), in the
dtype of their inputs, and a seeded case maker.  tests/golden/gru_*.npz (made from the reference's own modules by
tests/golden/make_gru_golden.py) pin the literal form; the GPU tests hold `FusedSepConvGRU` / `FusedConvGRU` against it in float64.

  literal_gru   the reference's forward, line by line, on its own state dict (`convz1.weight` ...): two `cat`s, three convolutions,
                two sigmoids, a tanh and the blend per half-step
  split_gru     the same function with every convolution split by input (h side, x side with the bias) and z, r merged:
                    convz(cat[h, x]) = Wz[:, :Ch] * h + Wz[:, Ch:] * x + bz        (a convolution is linear in its input channels)
                on the split parameters w_zr_h, w_zr_x, b_zr, w_q_h, w_q_x, b_q of `split_params`
  gate_forward, blend_forward, blend_backward, gate_backward
                the four formulas of the kernels (GgrGruPass in include/ggr_raster.h), on whole tensors"""
import torch
import torch.nn.functional as F

#        kind: [(suffix of the reference's module names, kernel shape, padding)] in the order the reference applies them
HALVES = {"sep": [("1", (1, 5), (0, 2)), ("2", (5, 1), (2, 0))], "conv": [("", (3, 3), (1, 1))]}
SPLIT = ("w_zr_h", "w_zr_x", "b_zr", "w_q_h", "w_q_x", "b_q")


def reference_keys(kind):
    return [f"conv{gate}{s}.{what}" for s, _, _ in HALVES[kind] for gate in "zrq" for what in ("weight", "bias")]


def split_names(kind):
    return [name + s for s, _, _ in HALVES[kind] for name in SPLIT]


def literal_gru(kind, sd, h, x):
    for s, _, pad in HALVES[kind]:
        conv = lambda gate, t: F.conv2d(t, sd[f"conv{gate}{s}.weight"], sd[f"conv{gate}{s}.bias"], padding=pad)
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(conv("z", hx))
        r = torch.sigmoid(conv("r", hx))
        q = torch.tanh(conv("q", torch.cat([r * h, x], dim=1)))
        h = (1 - z) * h + z * q
    return h


def split_params(kind, sd, ch):
    """The reference's tensors (parameters, or their gradients: the map is a selection) in the split layout."""
    out = {}
    for s, _, _ in HALVES[kind]:
        wz, wr, wq = (sd[f"conv{gate}{s}.weight"] for gate in "zrq")
        out["w_zr_h" + s] = torch.cat([wz[:, :ch], wr[:, :ch]], 0)
        out["w_zr_x" + s] = torch.cat([wz[:, ch:], wr[:, ch:]], 0)
        out["b_zr" + s] = torch.cat([sd[f"convz{s}.bias"], sd[f"convr{s}.bias"]], 0)
        out["w_q_h" + s], out["w_q_x" + s], out["b_q" + s] = wq[:, :ch], wq[:, ch:], sd[f"convq{s}.bias"]
    return out


def gate_forward(a_zr_h, a_zr_x, h):
    a = a_zr_h if a_zr_x is None else a_zr_h + a_zr_x
    ch = h.shape[1]
    z, r = torch.sigmoid(a[:, :ch]), torch.sigmoid(a[:, ch:])
    return z, r, r * h


def blend_forward(a_q_h, a_q_x, z, h):
    q = torch.tanh(a_q_h if a_q_x is None else a_q_h + a_q_x)
    return q, (1 - z) * h + z * q


def blend_backward(g, z, q, h):
    """-> dL/da_q, dL/da_z, dL/dh_part"""
    return g * z * (1 - q * q), g * (q - h) * z * (1 - z), g * (1 - z)


def gate_backward(g_rh, h, r, g_h_part=None):
    """-> dL/da_r, dL/dh (without what the w_zr_h convolution's input gradient adds)"""
    g_h = g_rh * r
    return g_rh * h * r * (1 - r), g_h if g_h_part is None else g_h_part + g_h


def split_gru(kind, p, h, x):
    for s, _, pad in HALVES[kind]:
        a_zr_h = F.conv2d(h, p["w_zr_h" + s], None, padding=pad)
        a_zr_x = F.conv2d(x, p["w_zr_x" + s], p["b_zr" + s], padding=pad)
        a_q_x = F.conv2d(x, p["w_q_x" + s], p["b_q" + s], padding=pad)
        z, _, rh = gate_forward(a_zr_h, a_zr_x, h)
        a_q_h = F.conv2d(rh, p["w_q_h" + s], None, padding=pad)
        _, h = blend_forward(a_q_h, a_q_x, z, h)
    return h


def make_gru_case(kind, N, ch, cx, H, W, seed):
    """Seeded float64 CPU inputs: the reference's state dict (uniform in +-1/sqrt(fan_in), as nn.Conv2d initialises, times 3 so that
    the gates leave the linear range), a hidden state in (-1, 1), features of unit scale and the upstream gradient `g`."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for s, (kh, kw), _ in HALVES[kind]:
        bound = 3.0 / ((ch + cx) * kh * kw) ** 0.5
        for gate in "zrq":
            sd[f"conv{gate}{s}.weight"] = (2 * torch.rand(ch, ch + cx, kh, kw, generator=gen, dtype=torch.float64) - 1) * bound
            sd[f"conv{gate}{s}.bias"] = (2 * torch.rand(ch, generator=gen, dtype=torch.float64) - 1) * bound
    return dict(sd=sd, h=torch.tanh(torch.randn(N, ch, H, W, generator=gen, dtype=torch.float64)),
                x=torch.randn(N, cx, H, W, generator=gen, dtype=torch.float64), g=torch.rand(N, ch, H, W, generator=gen, dtype=torch.float64) + 0.5)


def run_gru(route, kind, case, dtype, device, need=("h", "x", "params")):
    """`route`: "literal", "split", or a callable (hidden_dim, input_dim) -> a module with `load_reference_state_dict` whose
    parameters carry the split names (FusedSepConvGRU / FusedConvGRU).  The loss is sum(h' * g).  Returns detached results: out, g_h,
    g_x and g_<split name> for every split parameter — the literal route's parameter gradients are mapped to the split layout, which
    is a selection — each None where `need` leaves it out."""
    ch, cx = case["h"].shape[1], case["x"].shape[1]
    h, x, g = (case[k].detach().to(device=device, dtype=dtype).clone() for k in ("h", "x", "g"))
    h.requires_grad_("h" in need)
    x.requires_grad_("x" in need)
    sd = {k: v.detach().to(device=device, dtype=dtype).clone() for k, v in case["sd"].items()}
    if route == "literal":
        leaves = sd
        for v in sd.values():
            v.requires_grad_("params" in need)
        out = literal_gru(kind, sd, h, x)
    elif route == "split":
        leaves = {k: v.clone() for k, v in split_params(kind, sd, ch).items()}
        for v in leaves.values():
            v.requires_grad_("params" in need)
        out = split_gru(kind, leaves, h, x)
    else:
        module = route(ch, cx).to(device=device, dtype=dtype)
        module.load_reference_state_dict(sd)
        leaves = dict(module.named_parameters())
        assert sorted(leaves) == sorted(split_names(kind))
        for v in leaves.values():
            v.requires_grad_("params" in need)
        out = module(h, x)
    if need:
        (out * g).sum().backward()
    res = dict(out=out.detach(), g_h=h.grad, g_x=x.grad)
    if "params" in need:
        grads = {k: v.grad for k, v in leaves.items()}
        if route == "literal":
            grads = split_params(kind, grads, ch)
        res.update({"g_" + k: v.detach() for k, v in grads.items()})
    else:
        res.update({"g_" + k: None for k in split_names(kind)})
    return res


def result_keys(kind):
    return ["out", "g_h", "g_x"] + ["g_" + k for k in split_names(kind)]
