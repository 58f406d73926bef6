"""The five encoder passes — adapter, depth head, epipolar sampler and the two attention cores — on a stream other than the default
one, and captured into and replayed from a graph.

Every launch of theirs takes `torch.cuda.current_stream` (ggrt_official_amd/splatting.py) and hands it to the C entry point; the
sampler's backward is three kernels, the first of which zeroes an accumulator (`launch_epipolar_backward`, csrc/epipolar.hip), the attention launches
call `hipFuncSetAttribute` above 64 KiB of LDS (`allow_lds`, csrc/epipolar_attn.hip and epipolar_attn_enc.hip).  A launch or a
zeroing that went to the null stream instead is invisible to a test that only ever uses the default stream.

Side stream.  The stream is first kept busy for about a millisecond (2048² matmuls), then the pass's inputs are WRITTEN on it (copies
into buffers that held zeros), then the pass and its backward are called — nothing waits in between.  Work that slipped onto another
stream reads the zeros.  The result must equal the same call on the default stream: to the bit for everything documented as
reproducible (the adapter's outputs and per-Gaussian gradients, the depth head, both attention cores, the sampler's forward), to the
bar against float64 for the two sums made with float atomics (the adapter's per-camera gradients, the sampler's dL/dimages).

Graph.  Forward plus backward captured on a side stream with `torch.cuda.graph` after one uncaptured warm-up call there, then
replayed three times with new values copied into the static inputs; each replay must match an eager call on the same values under
the same rule.  The capture is one linear stream.

`fused_gaussian_adapter` and `fused_epipolar_sampler` begin with `torch.linalg.inv` of the cameras, which checks an error flag on
the host: it cannot be captured, and on a side stream it would wait for the stream and so hide what the test looks for.  Those two
are therefore entered at their autograd Functions (`_FusedAdapter`, `_FusedEpipolarSampler`) with the camera matrices prepared
beforehand; the depth head and the cores go through their public wrappers.  The adapter's per-camera gradients are taken to
extrinsics and intrinsics through torch's backward of that prelude afterwards, where `adapter_reference` has its float64 values.

Shapes: small ragged ones of the passes' own tests, and for the cores also S = 64, C = 256 (66 560 and, with 16 octaves, 74 752
bytes of LDS: the `hipFuncSetAttribute` path)."""
import pytest
import torch

from tests import test_gpu_adapter as A
from tests import test_gpu_depth_head as D
from tests import test_gpu_epipolar as E
from tests.adapter_reference import adapter_reference
from tests.adapter_reference import make_case as adapter_case
from tests.depth_head_reference import make_case as depth_head_case
from tests.encoder_cores import DEV, core_inputs, core_names, kernel_core, run_core_on
from tests.epipolar_reference import epipolar_reference
from tests.epipolar_reference import make_case as epipolar_case

pytestmark = pytest.mark.gpu

f32 = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()


def _bar(got, ref, t32, what):
    e_k, e_t = E._err(got, ref), E._err(t32, ref)
    print(f"{what} e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
    assert float(ref.abs().max()) > 0 and e_k <= max(4 * e_t, 1e-6), (what, e_k, e_t)


class _Adapter:
    exact = ("means", "scales", "quats", "harmonics", "d_depth", "d_coords", "d_raw")
    written = ("depths", "coordinates", "raw_gaussians")

    def __init__(self):
        from ggrt_official_amd import splatting
        self.fn = splatting._FusedAdapter
        self.case = adapter_case(3, 255, 3, 4, seed=700)
        self.weights = A._weights(adapter_reference(**self.case), 700)
        self.w = [f32(self.weights[k]) for k in A.OUTPUTS]
        # the prelude of fused_gaussian_adapter, once, with autograd on: its backward turns the Function's camera gradients into
        # those of extrinsics and intrinsics
        self.ext, self.intr = (f32(self.case[k]).requires_grad_(True) for k in ("extrinsics", "intrinsics"))
        h, w = self.case["image_shape"]
        pixel = torch.tensor([1.0 / w, 1.0 / h], dtype=torch.float32, device=DEV)
        mult = 0.1 * (torch.linalg.inv(self.intr[..., :2, :2]) @ pixel).sum(-1)
        self.prelude = (self.ext[..., :3, :4].contiguous(), torch.linalg.inv(self.intr), splatting.matrix_to_quaternion_wxyz(self.ext[..., :3, :3]), mult)
        self.cams = [t.detach().clone() for t in self.prelude] + [f32(self.case["sh_transform"])]
        self.mask = splatting.adapter_sh_mask(4, DEV)

    def values(self, i):
        fresh = adapter_case(3, 255, 3, 4, seed=700 + i)
        return {k: f32(fresh[k]) for k in self.written}

    def run(self, x):
        leaves = [x[k].detach().requires_grad_(True) for k in ("depths", "coordinates", "raw_gaussians")] + [t.detach().requires_grad_(True) for t in self.cams]
        out = self.fn.apply(*leaves, self.mask, self.case["scale_min"], self.case["scale_max"], 1e-8)
        grads = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, self.w)), leaves)
        names = ("means", "scales", "quats", "harmonics", "d_depth", "d_coords", "d_raw", "d_c2w", "d_kinv", "d_q", "d_mult", "d_sh_t")
        return dict(zip(names, tuple(o.detach() for o in out) + grads))

    def check_summed(self, i, got, what):
        case = dict(self.case, **{k: v.double().cpu() for k, v in self.values(i).items()})
        ref = A._run(adapter_reference, case, torch.float64, "cpu", self.weights)
        t32 = A._run(adapter_reference, case, torch.float32, DEV, self.weights)
        d_ext, d_intr = torch.autograd.grad(self.prelude, [self.ext, self.intr], [got[k] for k in ("d_c2w", "d_kinv", "d_q", "d_mult")], retain_graph=True)
        for k, g in (("d_extrinsics", d_ext), ("d_intrinsics", d_intr), ("d_sh_transform", got["d_sh_t"])):
            _bar(g.double().cpu(), ref[k], t32[k], f"{what} adapter {k}")


class _DepthHead:
    exact = ("depths", "opacities", "coordinates", "index", "d_logits", "d_xy_raw")
    written = ("logits", "xy_raw")

    def __init__(self):
        self.case = depth_head_case(3, 65, 32, 1, 3, "sampled", seed=710, use_transmittance=True, opacity_exponent=2 ** 0.5)
        self.fixed = {k: (f32(v) if torch.is_tensor(v) else v) for k, v in self.case.items() if k not in self.written}
        self.w = {k: f32(v) for k, v in D._weights(self.case, 710).items()}

    def values(self, i):
        fresh = depth_head_case(3, 65, 32, 1, 3, "sampled", seed=710 + i, use_transmittance=True, opacity_exponent=2 ** 0.5)
        return {k: f32(fresh[k]) for k in self.written}

    def run(self, x):
        from ggrt_official_amd import fused_depth_head
        leaves = [x[k].detach().requires_grad_(True) for k in self.written]
        out = fused_depth_head(logits=leaves[0], xy_raw=leaves[1], **self.fixed)
        grads = torch.autograd.grad(sum((getattr(out, k) * self.w[k]).sum() for k in D.OUTPUTS), leaves)
        return dict(depths=out.depths.detach(), opacities=out.opacities.detach(), coordinates=out.coordinates.detach(), index=out.index,
                    d_logits=grads[0], d_xy_raw=grads[1])

    def check_summed(self, i, got, what):
        pass


class _Sampler:
    exact = ("features", "valid", "xy_ray", "xy_sample", "xy_sample_near", "xy_sample_far", "origins", "directions", "depth")
    written = ("images",)

    def __init__(self):
        from ggrt_official_amd import splatting
        self.fn = splatting._FusedEpipolarSampler
        self.case = epipolar_case(1, 3, 11, 13, 5, 8, 720)
        self.weights = E._weights(self.case, 720)
        self.w = f32(self.weights)
        c2w, K = f32(self.case["extrinsics"]), f32(self.case["intrinsics"])
        self.cams = (c2w, torch.linalg.inv(c2w).contiguous(), K, torch.linalg.inv(K).contiguous(), f32(self.case["near"]), f32(self.case["far"]))
        self.dims = (1, 3, 5, 11, 13, 8, None)

    def _images(self, i):
        return torch.randn(self.case["images"].shape, generator=torch.Generator().manual_seed(720 + i), dtype=torch.float64)

    def values(self, i):
        return {"images": f32(self._images(i))}

    def run(self, x):
        images = x["images"].detach().requires_grad_(True)
        out = self.fn.apply(images, *self.cams, self.dims)
        (g,) = torch.autograd.grad((out[0] * self.w).sum(), [images])
        return dict(zip(self.exact, (out[0].detach(),) + tuple(out[1:])), d_images=g)

    def check_summed(self, i, got, what):
        case = dict(self.case, images=self._images(i))
        ref = E._run(epipolar_reference, case, torch.float64, "cpu", self.weights)
        t32 = E._run(epipolar_reference, case, torch.float32, DEV, self.weights)
        assert torch.equal(got["valid"].bool().cpu(), ref["valid"])
        _bar(got["d_images"].double().cpu(), ref["d_images"], t32["d_images"], f"{what} sampler d_images")


class _Core:
    def __init__(self, n, s, c, h, octaves):
        self.shape, self.octaves = (n, s, c, h), octaves
        self.encoded = octaves is not None
        self.exact = core_names(self.encoded)
        self.written = ("qk", "qe", "f", "d") if self.encoded else ("qk", "z")
        t = core_inputs(n, s, c, h, 730, octaves)
        self.grads = [f32(t[k]) for k in (("g_ctx_f", "g_ctx_e") if self.encoded else ("g_ctx",))]

    def values(self, i):
        t = core_inputs(*self.shape, 730 + i, self.octaves)
        return {k: f32(t[k]) for k in self.written}

    def run(self, x):
        return dict(zip(self.exact, run_core_on(kernel_core(self.encoded), [x[k] for k in self.written], self.grads)))

    def check_summed(self, i, got, what):
        pass


PASSES = {"adapter": _Adapter, "depth_head": _DepthHead, "sampler": _Sampler,
          "attention": lambda: _Core(3, 33, 130, 8, None), "attention_lds": lambda: _Core(2, 64, 256, 8, None),
          "encoded_attention": lambda: _Core(3, 33, 130, 8, 5), "encoded_attention_lds": lambda: _Core(2, 64, 256, 8, 16)}


def _same(p, i, got, want, what):
    assert set(got) == set(want) and set(p.exact) <= set(got)
    for k in p.exact:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert float(want[k].double().abs().max()) > 0, (what, k)
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs from the default stream's in {int((got[k] != want[k]).sum())} of {got[k].numel()} elements"
    p.check_summed(i, want, what + " (default stream)")
    p.check_summed(i, got, what)


@pytest.mark.parametrize("name", list(PASSES))
def test_a_pass_on_a_busy_side_stream_equals_the_default_stream(name):
    p = PASSES[name]()
    src = p.values(1)
    want = p.run(src)
    busy = torch.randn(2048, 2048, device=DEV)
    (busy @ busy).sum().item()                       # (the BLAS library is initialised before the stream section)
    static = {k: torch.zeros_like(v) for k, v in src.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        for _ in range(10):
            busy @ busy
        for k, v in src.items():
            static[k].copy_(v, non_blocking=True)
        got = p.run(static)
    torch.cuda.synchronize()
    _same(p, 1, got, want, f"side stream, {name}")


@pytest.mark.parametrize("name", list(PASSES))
def test_a_captured_pass_replays_with_new_values(name):
    """The sampler's case found a defect: `launch_epipolar_backward` zeroed its accumulator with `hipMemsetAsync`, and a replay of
    the captured backward that came after an eager sampler call returned dL/dimages with e_kernel 1.562e+15 (every second or fourth
    element wrong; the replays before any eager call were right).  The accumulator is now zeroed by a kernel
    (`epipolar_zero_kernel`), a graph node like the launches around it."""
    p = PASSES[name]()
    static = {k: v.clone() for k, v in p.values(0).items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        p.run(static)                                # the warm-up, uncaptured
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = p.run(static)
    torch.cuda.synchronize()
    for i in (1, 2, 3):
        fresh = p.values(i)
        for k, v in fresh.items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        want = p.run(fresh)
        torch.cuda.synchronize()
        _same(p, i, got, want, f"replay {i}, {name}")
