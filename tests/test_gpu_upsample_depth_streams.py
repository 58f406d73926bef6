"""`fused_upsample_depth` off the default stream and inside a training step's traffic: on a side stream that is busy with other
work, on two side streams at once, interleaved with a call of another shape so that torch's caching allocator hands one call's
freed workspace (`up` forward, the tap sums [N,9,h,w] backward) to the next, and from a replayed `torch.cuda.graph` whose inputs
were refreshed twice.  The pass works on the caller's stream, allocates nothing itself, never synchronises and sums in a fixed
order, so every comparison here is to the bit."""
import pytest
import torch

import ggrt_official_amd.splatting as splatting
from tests.test_upsample_depth_reference import DISP_RANGE, RESIZE_CASES
from tests.upsample_depth_reference import make_upsample_case, run_upsample_depth

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("out", "g_depth", "g_mask")


@pytest.fixture(autouse=True)
def _poison():
    splatting._IMAGE_LOSS_POISON = True
    yield
    splatting._IMAGE_LOSS_POISON = False


def _ker(*args, **kw):
    from ggrt_official_amd import fused_upsample_depth
    return fused_upsample_depth(*args, **kw)


def _case(name, seed=None):
    N, h, w, r, size, s = RESIZE_CASES[name]
    return make_upsample_case(N, h, w, r, size, s if seed is None else seed), dict(ratio=r, image_size=size, disp_range=DISP_RANGE)


def _same(got, want, what):
    for k in KEYS:
        assert not torch.isnan(got[k]).any() and torch.equal(got[k], want[k]), (what, k)


def _busy(a):
    for _ in range(8):
        a = (a @ a).clamp(-1, 1)
    return a


def test_on_a_busy_side_stream():
    case, opts = _case("seams_r3")
    plain = run_upsample_depth(_ker, case, torch.float32, DEV, **opts)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = _busy(a)            # work in front of the pass on its own stream, and behind it
        got = run_upsample_depth(_ker, case, torch.float32, DEV, **opts)
        a = _busy(a)
    side.synchronize()
    _same(got, plain, "side stream")


def test_on_two_side_streams_at_once():
    (case_a, opts), (case_b, _) = _case("seams_r3", 980), _case("seams_r3", 981)
    serial = [run_upsample_depth(_ker, c, torch.float32, DEV, **opts) for c in (case_a, case_b)]
    assert not torch.equal(serial[0]["out"], serial[1]["out"])
    torch.cuda.synchronize()
    streams, got = [torch.cuda.Stream(), torch.cuda.Stream()], [None, None]
    a = [torch.randn(1024, 1024, device=DEV) for _ in streams]
    torch.cuda.synchronize()
    for i, (s, c) in enumerate(zip(streams, (case_a, case_b))):
        with torch.cuda.stream(s):
            a[i] = _busy(a[i])          # (keeps the first stream occupied while the second is being fed)
            got[i] = run_upsample_depth(_ker, c, torch.float32, DEV, **opts)
    torch.cuda.synchronize()
    for i in range(2):
        _same(got[i], serial[i], f"stream {i}")


def _forward(case, opts):
    t = {k: v.to(device=DEV, dtype=torch.float32).clone() for k, v in case.items()}
    depth, mask = t["depth"].requires_grad_(True), t["mask"].requires_grad_(True)
    return depth, mask, t["g"], _ker(depth, mask, **opts)


def _backward(depth, mask, g, out):
    g_depth, g_mask = torch.autograd.grad((out * g).sum(), (depth, mask))
    return dict(out=out.detach(), g_depth=g_depth, g_mask=g_mask)


def test_interleaved_calls_of_two_shapes_and_a_reused_workspace():
    (case_a, opts_a), (case_b, opts_b) = _case("seams_r8_resized"), _case("strong_up")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    alone_a = run_upsample_depth(_ker, case_a, torch.float32, DEV, **opts_a)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    alone_b = run_upsample_depth(_ker, case_b, torch.float32, DEV, **opts_b)
    # forward A, forward B, backward A, backward B
    fa, fb = _forward(case_a, opts_a), _forward(case_b, opts_b)
    got_a, got_b = _backward(*fa), _backward(*fb)
    _same(got_a, alone_a, "A between B's halves")
    _same(got_b, alone_b, "B around A's backward")
    del fa, fb, got_a, got_b
    # forward A, backward A, A's tensors dropped (no empty_cache: B's buffers may be A's freed blocks), forward B, backward B
    fa = _forward(case_a, opts_a)
    got_a = {k: v.cpu() for k, v in _backward(*fa).items()}
    del fa
    got_b = _backward(*_forward(case_b, opts_b))
    _same(got_a, {k: v.cpu() for k, v in alone_a.items()}, "A before B")
    _same(got_b, alone_b, "B in A's freed blocks")


def test_graph_replay_with_two_refreshes():
    """Forward + backward captured once; replayed with the second inputs, then with the first again, the outputs NaN before each."""
    first, opts = _case("one_smaller", 982)
    second, _ = _case("one_smaller", 983)
    eager = {id(c): run_upsample_depth(_ker, c, torch.float32, DEV, **opts) for c in (first, second)}
    assert not torch.equal(eager[id(first)]["out"], eager[id(second)]["out"])
    t = {k: v.to(device=DEV, dtype=torch.float32).clone() for k, v in first.items()}
    depth, mask, g = t["depth"].requires_grad_(True), t["mask"].requires_grad_(True), t["g"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # (warm-up on a side stream, as torch's graph recipe asks)
        for _ in range(2):
            torch.autograd.grad((_ker(depth, mask, **opts) * g).sum(), (depth, mask))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _ker(depth, mask, **opts)
        g_depth, g_mask = torch.autograd.grad((out * g).sum(), (depth, mask))
    for case in (second, first):
        with torch.no_grad():
            for k, dst in (("depth", depth), ("mask", mask), ("g", g)):
                dst.copy_(case[k].to(device=DEV, dtype=torch.float32))
            for buf in (out, g_depth, g_mask):
                buf.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same(dict(out=out.detach(), g_depth=g_depth, g_mask=g_mask), eager[id(case)], "replay")
