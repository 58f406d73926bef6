"""Shared by the encoder passes' second-layer tests (buffers, streams, inputs): seeded inputs of the two attention cores and one
forward + backward of a core on the device, for the tests that compare a run of the kernels with another run of theirs."""
import torch

DEV = "cuda:0"
PLAIN = ("qk", "z")
ENCODED = ("qk", "qe", "f", "d")


def core_inputs(n, s, c, h, seed, octaves=None):
    """float64 CPU inputs and upstream gradients of `epipolar_attention_core` (octaves None) or of
    `epipolar_encoded_attention_core`; the depths are float32 numbers in [0, 1], as the sampler's are"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    if octaves is None:
        return dict(qk=0.3 * r(n, h, c), z=r(n, s, c), g_ctx=r(n, h, c))
    return dict(qk=0.3 * r(n, h, c), qe=0.3 * r(n, h, 2 * octaves), f=r(n, s, c), d=torch.rand((n, s), generator=gen, dtype=torch.float32).double(),
                g_ctx_f=r(n, h, c), g_ctx_e=r(n, h, 2 * octaves))


def kernel_core(encoded):
    from ggrt_official_amd import epipolar_attention_core, epipolar_encoded_attention_core
    return epipolar_encoded_attention_core if encoded else epipolar_attention_core


def run_core_on(fn, leaves, grads):
    """`fn(*leaves)` → (…, attn) and the gradients of all leaves for the upstream `grads`, on the leaves' device, as they come"""
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    *ctx, attn = fn(*leaves)
    got = torch.autograd.grad(ctx, leaves, grads)
    return tuple(c.detach() for c in ctx) + (attn.detach(),) + tuple(got)


def core_names(encoded):
    return ("ctx_f", "ctx_e", "attn", "g_qk", "g_qe", "g_f", "g_d") if encoded else ("ctx", "attn", "g_qk", "g_z")
