"""`fused_image_loss` on a stream other than the default one, and captured into and replayed from a graph (the pattern of
tests/test_gpu_encoder_streams.py).

Every launch takes `torch.cuda.current_stream` and hands it to the C entry point; the pass sets no memory (its partial sums are
written whole by the forward's workgroups and added by a finishing launch on the same stream).  A launch that went to the null
stream instead is invisible to a test that only ever uses the default stream.

Side stream: the stream is first kept busy for about a millisecond (2048² matmuls), then the images are WRITTEN on it (copies into
buffers that held zeros), then forward and backward are called — nothing waits in between.  Graph: forward plus backward captured on
a side stream after one uncaptured warm-up there AND an eager call on the default stream (the order that showed the sampler's
`hipMemsetAsync` defect), replayed three times with new values copied into the static inputs.  Everything — both results and both
gradients — must equal the eager default-stream call to the bit: the pass has no atomics.

Shapes: [2, 3, 33, 65] (several tiles each way, ragged edges) with a mask and per-image results, and [1, 3, 20, 40] without."""
import pytest
import torch

from tests.image_loss_reference import make_image_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

f32 = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()


class _Loss:
    written = ("pred", "target")

    def __init__(self, b, c, h, w, masked, size_average, window_size):
        self.shape, self.masked, self.size_average, self.window_size = (b, c, h, w), masked, size_average, window_size
        case = make_image_case(b, c, h, w, 0.1, 1200, masked)
        self.mask = f32(case["mask"]) if masked else None
        n = 1 if size_average else b
        self.g = (f32(case["g_mse"])[:n], f32(case["g_ssim"])[:n])

    def values(self, i):
        case = make_image_case(*self.shape, 0.1, 1200 + i, self.masked)
        return {k: f32(case[k]) for k in self.written}

    def run(self, x):
        from ggrt_official_amd import fused_image_loss
        pred, target = (x[k].detach().requires_grad_(True) for k in self.written)
        out = fused_image_loss(pred, target, self.mask, window_size=self.window_size, size_average=self.size_average)
        d_pred, d_target = torch.autograd.grad((out.mse.reshape(-1) * self.g[0]).sum() + (out.ssim.reshape(-1) * self.g[1]).sum(), [pred, target])
        return dict(mse=out.mse.detach(), ssim=out.ssim.detach(), d_pred=d_pred, d_target=d_target)


PASSES = {"masked_per_image": lambda: _Loss(2, 3, 33, 65, True, False, 11), "plain_mean_window7": lambda: _Loss(1, 3, 20, 40, False, True, 7)}


def _same(got, want, what):
    assert set(got) == set(want) == {"mse", "ssim", "d_pred", "d_target"}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert torch.isfinite(want[k]).all() and float(want[k].abs().max()) > 0, (what, k)
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs from the default stream's in {int((got[k] != want[k]).sum())} of {got[k].numel()} elements"


@pytest.mark.parametrize("name", list(PASSES))
def test_the_loss_on_a_busy_side_stream_equals_the_default_stream(name):
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
    _same(got, want, f"side stream, {name}")


@pytest.mark.parametrize("name", list(PASSES))
def test_a_captured_loss_replays_with_new_values_after_an_eager_call(name):
    p = PASSES[name]()
    static = {k: v.clone() for k, v in p.values(0).items()}
    p.run(p.values(4))                               # an eager call on the default stream comes first
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
        want = p.run(fresh)                          # (eager calls between the replays too)
        torch.cuda.synchronize()
        _same(got, want, f"replay {i}, {name}")
