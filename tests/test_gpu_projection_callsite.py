"""`return_projection` through the call-site layer on the GPU (`-m gpu`): the fused render functions and `DecoderSplattingCUDA`
pass the keyword on wherever they pass `return_hits`, put the `Projection` behind everything else, stack per-call results like
the hits ([b,v,g,…] in `DecoderOutput.projection`), change nothing in front of it, and keep it differentiable."""
import pytest
import torch

from ggrt_official_amd import PixelHits, Projection
from ggrt_official_amd import splatting as S
from tests.helpers import GRAD_RTOL, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = Projection._fields[:5]


def _case(grad=False):
    gen = torch.Generator().manual_seed(2301)
    b, v, n, d_sh, h, w = 2, 2, 1500, 9, 64, 96
    ext = torch.eye(4).repeat(b, v, 1, 1)
    ext[..., 0, 3] = torch.linspace(-0.2, 0.2, v)
    Kmat = torch.tensor([[1.0, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).repeat(b, v, 1, 1)
    near, far = torch.full((b, v), 0.5), torch.full((b, v), 50.0)
    means = torch.randn(b, n, 3, generator=gen) * torch.tensor([0.6, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.0])
    means[:, -4:, 2] = -1.0     # four behind the camera …
    means[:, -8:-4, 0] = 300.0  # … and four far outside the frustum, per batch element
    A = torch.randn(b, n, 3, 3, generator=gen) * 0.05
    cov = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3)
    harm = torch.randn(b, n, 3, d_sh, generator=gen) * 0.3
    opac = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    to = (lambda t: t.to(DEV).requires_grad_(True)) if grad else (lambda t: t.to(DEV))
    gs = S.Gaussians(to(means), to(cov), to(harm), to(opac))
    return gs, (gs, ext.to(DEV), Kmat.to(DEV), near.to(DEV), far.to(DEV), (h, w)), (b, v, n, h, w)


def _same(a, b, tag):
    for f in Projection._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), (tag, f)


def test_decoder_projection_equals_per_view_calls_on_every_path():
    gs, args, (b, v, n, h, w) = _case()
    dec = S.DecoderSplattingCUDA(sh_max_degree=3).to(DEV)
    with torch.no_grad():
        plain = dec(*args, depth_mode="depth")
        out = dec(*args, depth_mode="depth", return_projection=True)
        assert plain.projection is None and out.hits is None and isinstance(out.projection, Projection)
        p = out.projection
        assert [tuple(t.shape) for t in p] == [(b, v, n, 2), (b, v, n), (b, v, n, 3), (b, v, n), (b, v, n, 3), (b, v, n)]
        assert torch.equal(out.color, plain.color) and torch.equal(out.depth, plain.depth)
        assert not bool(p.valid[:, :, -8:].any()) and int(p.valid.sum()) > b * v * n // 2
        for f in FLOATS:
            assert not bool(getattr(p, f)[~p.valid].any()), f
        flat = lambda t: t.flatten(0, 1)
        bg = torch.zeros(b * v, 3, device=DEV)
        per_view = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w), bg, gs,
                                        [n_ // v for n_ in range(b * v)], "depth", batched=False, sh_max_degree=3,
                                        return_projection=True)
        assert len(per_view) == 3 and isinstance(per_view[-1], Projection)
        _same(Projection(*(flat(t) for t in p)), per_view[-1], "decoder (launch set) against per-view calls")
        # with the hits, picks, contributions and alpha as well: each in its place, the projection last
        every = dec(*args, depth_mode="depth", return_projection=True, return_hits=4, return_picks=True, return_contributions=True,
                    return_alpha=True)
        _same(every.projection, p, "decoder, with everything else")
        assert isinstance(every.hits, PixelHits) and torch.equal(every.hits.count, every.picks.count) and every.alpha is not None
        # one batch element at a time (the per-batch launch sets of render_views_fused)
        one = S.render_views_fused(flat(args[1])[:v], flat(args[2])[:v], args[3].flatten()[:v], args[4].flatten()[:v], (h, w),
                                   bg[:v], S.Gaussians(gs.means[:1], gs.covariances[:1], gs.harmonics[:1], gs.opacities[:1]),
                                   [0] * v, "depth", sh_max_degree=3, return_projection=True, return_hits=2)
        assert isinstance(one[-1], Projection) and isinstance(one[-2], PixelHits)
        _same(one[-1], Projection(*(t[0] for t in p)), "one batch element")
        # the reference-shaped call site takes the keyword too, with and without a depth pass.  It feeds the rasterizer other
        # input forms (scaled copies of the Gaussians), so its fields agree with the fused path's to rounding, not to the bit;
        # its depth value is the depth pass's per-Gaussian feature when a fused depth pass runs, view z otherwise
        slow = S.DecoderSplattingCUDA(sh_max_degree=3, fused_inputs=False).to(DEV)
        o2 = slow(*args, depth_mode="depth", return_projection=True)
        o3 = slow(*args, return_projection=True, return_hits=2, return_alpha=True)
        assert torch.equal(o2.projection.valid, p.valid) and torch.equal(o3.projection.valid, p.valid)
        assert o3.hits is not None and o3.alpha is not None and o2.hits is None
        for f in ("means2d", "conic", "opacity", "color"):
            assert torch.equal(getattr(o2.projection, f), getattr(o3.projection, f)), f
            assert torch.allclose(getattr(o2.projection, f), getattr(p, f), rtol=1e-3, atol=1e-3), f
        assert torch.allclose(o2.projection.depth, p.depth, rtol=1e-4, atol=1e-4)


def test_decoder_projection_is_differentiable_and_equals_the_per_view_sum():
    gs, args, (b, v, n, h, w) = _case(grad=True)
    gen = torch.Generator().manual_seed(2302)
    g = {f: torch.randn((b, v, n) + tail, generator=gen).to(DEV) for f, tail in zip(FLOATS, ((2,), (), (3,), (), (3,)))}
    dec = S.DecoderSplattingCUDA(sh_max_degree=3).to(DEV)
    out = dec(*args, depth_mode="depth", return_projection=True)
    assert all(getattr(out.projection, f).requires_grad for f in FLOATS) and not out.projection.valid.requires_grad
    sum((getattr(out.projection, f) * g[f]).sum() for f in FLOATS).backward()
    leaves = dict(means=gs.means, covariances=gs.covariances, harmonics=gs.harmonics, opacities=gs.opacities)
    got = {k: t.grad.clone() for k, t in leaves.items()}
    for t in leaves.values():
        t.grad = None
    flat = lambda t: t.flatten(0, 1)
    pv = S.render_views_fused(flat(args[1]), flat(args[2]), args[3].flatten(), args[4].flatten(), (h, w),
                              torch.zeros(b * v, 3, device=DEV), gs, [n_ // v for n_ in range(b * v)], "depth", batched=False,
                              sh_max_degree=3, return_projection=True)[-1]
    sum((getattr(pv, f) * flat(g[f])).sum() for f in FLOATS).backward()
    for k, t in leaves.items():
        r = rel_l2(got[k].cpu().numpy(), t.grad.cpu().numpy())
        print(f"decoder projection grad {k}: rel-L2 {r:.3e}")
        assert float(t.grad.abs().max()) > 0 and bool(torch.isfinite(got[k]).all()) and r <= GRAD_RTOL, k
