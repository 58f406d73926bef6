"""Every element of every buffer that the adapter, the epipolar sampler and the two attention cores return is WRITTEN by their
kernels, whatever the buffer held before.

The comparisons of tests/test_gpu_adapter.py, test_gpu_epipolar.py and test_gpu_epipolar*_attention.py run the float32 torch route
on the device right before the kernels, at the same shapes; the wrappers take their outputs from `torch.empty`, and the caching
allocator may hand them the very blocks that still hold the torch route's (right) answer — an element a kernel forgot would pass.
Here `torch.empty` and `torch.empty_like` are replaced, within the test only (pytest's monkeypatch: restored on exit), by versions
that fill what they return with NaN (0xFF bytes for integer and uint8 buffers); the references were computed before.  Every
returned tensor and every gradient must then be finite everywhere — asserted first, because NaN fails the bar's `<=` without
saying which write is missing — and hold the bar against float64.

Exempt, and why: the sampler's backward scratch (the channel-last accumulator of dL/dimages) is zeroed by the launch itself
(`epipolar_zero_kernel` in `launch_epipolar_backward`) before `epipolar_bwd_kernel` adds into it, so what it held cannot matter.  NOT
exempt: the forward scratch (the channel-last copy of the maps, written whole by `epipolar_to_channel_last_kernel` and read by every
tap: a missed element reaches `features` as NaN) and `segment` (read by the backward).  The adapter's per-camera gradients are
`torch.zeros_like` by design (the kernel adds into them).

The shapes are the ragged ones: the stores under test are
  adapter    `for (i = lane; i < nrows * S::W; …) dst[i] = …` (dL/draw) and `for (i = lane; i < cnt * S::H; …) dst[i] = …`
             (harmonics) with nrows < 64: G/spp = 85 (64 + 21) and 257 (4·64 + 1) rows, and a single row
  sampler    `if (c0 + k < a.c)` / `if (p0 + k < hw)` of the two layout kernels with c = 33 and h·w = 195 (32 + 1, 6·32 + 3), c = 1
             and h·w = 1; `for (ch = lane; ch < c; …)` and `if (lane < s)` of `epipolar_fwd_kernel` with c = s = 33
  cores      `for (c = lane; c < C; …)` with C = 130 (2·64 + 2), the `C & 3` element loads, `if (lane < S)` with S = 33 and 1, and the
             encoded core's `v >= C` columns with C + E = 140 and 288"""
import functools

import pytest
import torch

from tests import test_gpu_adapter as A
from tests import test_gpu_epipolar as E
from tests import test_gpu_epipolar_attention as P
from tests import test_gpu_epipolar_encoded_attention as N
from tests.encoder_cores import DEV

pytestmark = pytest.mark.gpu


def _poison(monkeypatch):
    real = {name: getattr(torch, name) for name in ("empty", "empty_like")}

    def filled(name):
        @functools.wraps(real[name])
        def make(*args, **kwargs):
            t = real[name](*args, **kwargs)
            if t.is_floating_point():
                t.fill_(float("nan"))
            elif t.dtype == torch.bool:
                t.fill_(True)
            else:
                t.fill_(0xFF if t.dtype == torch.uint8 else -1)
            return t
        return make

    for name in real:
        monkeypatch.setattr(torch, name, filled(name))
    probe = torch.empty((3,), device=DEV), torch.empty_like(torch.zeros(3, device=DEV)), torch.empty((2,), dtype=torch.uint8, device=DEV)
    assert bool(probe[0].isnan().all()) and bool(probe[1].isnan().all()) and probe[2].tolist() == [255, 255]


def _all_finite(res, what):
    for k, v in res.items():
        if torch.is_tensor(v) and v.is_floating_point():
            bad = int((~torch.isfinite(v)).sum())
            assert bad == 0, f"{what}: {bad} of {v.numel()} elements of {k} were never written"


@pytest.mark.parametrize("n_cam,g,spp,d_sh", [(3, 255, 3, 25), (3, 257, 1, 4), (1, 1, 1, 1)])
def test_the_adapter_writes_every_element(monkeypatch, n_cam, g, spp, d_sh):
    from ggrt_official_amd import fused_gaussian_adapter
    case, ref, t32, _ = A._routes(n_cam, g, spp, d_sh)
    weights = A._weights(ref, 7 * n_cam + g + 13 * spp + d_sh)
    _poison(monkeypatch)
    ker = A._run(fused_gaussian_adapter, case, torch.float32, DEV, weights)
    monkeypatch.undo()
    assert set(ker) == set(ref)
    _all_finite(ker, f"adapter C={n_cam} G={g} spp={spp} d_sh={d_sh}")
    A._hold_to_the_bar(ref, t32, ker, f"poisoned adapter C={n_cam} G={g} spp={spp} d_sh={d_sh}")


@pytest.mark.parametrize("h,w,c,s,window", [(65, 3, 33, 33, None), (1, 1, 1, 8, None), (16, 16, 6, 8, (3, 12, 2, 15))])
def test_the_sampler_writes_every_element(monkeypatch, h, w, c, s, window):
    from ggrt_official_amd import fused_epipolar_sampler
    case, ref, t32, _ = E._routes(1, 2, h, w, c, s, "default", window)
    seed = 3 * 1 + 5 * 2 + 7 * h + 11 * w + 13 * c + 17 * s
    _poison(monkeypatch)
    ker = E._run(fused_epipolar_sampler, case, torch.float32, DEV, E._weights(case, seed))
    monkeypatch.undo()
    _all_finite(ker, f"sampler {h}x{w} c={c} s={s} window={window}")
    E._hold_to_the_bar(ref, t32, ker, f"poisoned sampler {h}x{w} c={c} s={s} window={window}")


@pytest.mark.parametrize("n,s,dim,c,h,d,octaves", [(3, 33, 5, 130, 8, 1, None), (5, 1, 6, 1, 1, 3, None), (2, 64, 6, 256, 8, 2, None),
                                                   (3, 33, 5, 130, 8, 1, 5), (5, 1, 6, 1, 1, 3, 1), (2, 64, 6, 256, 8, 2, 16)])
def test_the_attention_cores_write_every_element(monkeypatch, n, s, dim, c, h, d, octaves):
    """(N, S, C, H[, O]) with the smallest projections around the cores (dim <= 6, D <= 3), as the cores' own tests have them: the
    literal restatement of the reference's attention is what the bar is defined against.  The cores' buffers (ctx, attn, dL/dqk,
    dL/dz or dL/dfeatures, dL/dqe, dL/ddepth) are the only `torch.empty` of these routes; a missed element of ctx or of a gradient
    reaches the output or a leaf's gradient through a GEMM, and `attn` is returned as it is."""
    if octaves is None:
        from ggrt_official_amd import fused_epipolar_attention as fused
        case, ref, t32, _ = P._routes(n, s, dim, c, h, d)
        run = lambda: P.run_route(fused, case, torch.float32, DEV)
        weights = lambda: fused(*[case[k].to(device=DEV, dtype=torch.float32) for k in ("x", "z", "w_q", "w_kv", "w_out", "b_out")], h, return_weights=True)[1]
        hold = P._hold_to_the_bar
    else:
        from ggrt_official_amd import fused_epipolar_encoded_attention as fused
        case, ref, t32, _ = N._routes(n, s, dim, c, h, d, octaves)
        run = lambda: N.run_enc_route(fused, case, torch.float32, DEV)
        weights = lambda: fused(*[case[k].to(device=DEV, dtype=torch.float32) for k in N.ENC_LEAVES], h, return_weights=True)[1]
        hold = N._hold_to_the_bar
    _poison(monkeypatch)
    ker = run()
    attn = weights().double().cpu()
    monkeypatch.undo()
    what = f"attention N={n} S={s} C={c} H={h} O={octaves}"
    _all_finite(dict(ker, attn=attn), what)
    assert attn.shape == (n, h, s) and float((attn.sum(-1) - 1).abs().max()) <= 1e-6
    hold(ref, t32, ker, "poisoned " + what, may_be_zero=("x", "w_q") if s == 1 else ())
