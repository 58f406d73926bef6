"""The intrinsics gradient on the GPU: dL/dtan(fov/2) from the backward (GgrBackwardExtra2.dL_dtanfov) against fp64 autograd of
the torch oracle, across launch sets and Gaussian sets; `camera_setup`'s backward (ggr_camera_setup_backward) against fp64
autograd of tests/camera_reference.py; the call site with poses and intrinsics that require grad, end to end and replayed
from a HIP graph.

dL/dtanfov, the references' own spread.  The two sums can cancel (on the 101×67 frame the Gaussians beyond the frustum clamp
contribute 2–2.5 × the total's norm, with the opposite sign of the rest), so the seeds of tests/tanfov_reference.py were chosen
with the oracle's fp32-against-fp64 rel-L2 on dL/dtanfov measured on the CPU in EVERY case of `test_dtanfov_matches_the_oracle`:
largest 1.40e-4 (80×48, D = 1, colour + depth, anti-aliased) — 0.07 of the 2e-3 bar, below the quarter asked for; without
anti-aliasing the largest is 9.0e-6.  tests/test_intrinsics_grad_abi.py measures one case per frame again on every run.

`camera_setup` backward, the bar.  The forward's fp32 outputs differ from the float64 reference by rel-L2 6e-8 … 1e-7 per output
tensor on these inputs (rounded to fp32 once, and 1/near, near·s, far·s, t·s in fp32 as the reference's call site has them; the
test measures the figure anew on every run, from the unchanged forward kernel, and prints it); the gradients are rounded once
as well and are allowed 4 × the largest of those figures."""
import numpy as np
import pytest
import torch

from ggrt_official_amd.synthetic import make_scene, upstream_gradient
from oracle import torch_raster as tr
from tests import camera_reference as cr
from tests import camera_scenes as cs_
from tests import tanfov_reference as R
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _leaf(t):
    return t.detach().clone().to(dev).requires_grad_(True)


QUAD = (slice(16, 24), slice(32, 40))   # one 8×8 quadrant (one wave of the blend backward) in the dense middle of every frame here


def _one_quadrant(t):
    """`t` [..., H, W] with everything outside QUAD zeroed.  The blend backward commits one float atomic per (wave, Gaussian,
    record slot), so two identical full-frame backwards differ in their last bits (tests/test_gpu_hits_grad.py: rel-L2 below
    4e-8); with the loss confined to one wave's pixels every record receives ONE non-zero addend (the others add exact zeros)
    and nothing depends on the order — the setting in which "bit for bit" can be asked of two backwards (checked when this test
    was written: the same call twice gave max |Δ| = 0 on every gradient in all 24 cases)."""
    if t is None:
        return None
    m = torch.zeros_like(t)
    m[..., QUAD[0], QUAD[1]] = t[..., QUAD[0], QUAD[1]]
    return m


def _hip(frame, D, loss, antialiasing, want_fov, one_quadrant=False):
    """GaussianRasterizer on the case's scene, scale + rotation inputs, camera tensors as leaves, settings.tanfov a device [2]
    tensor that requires grad or not: dict of numpy gradients"""
    from ggrt_official_amd import GaussianRasterizer
    cs = R.scene(frame, D)
    sc = cs.sc
    dL, dLd, dLa = R.upstream(frame, loss)
    if one_quadrant:
        dL, dLd, dLa = _one_quadrant(dL), _one_quadrant(dLd), _one_quadrant(dLa)
    leaves = {k: _leaf(getattr(sc, k)) for k in R.GAUSSIAN_KEYS + R.CAMERA_KEYS}
    tf = torch.tensor([sc.tanfovx, sc.tanfovy], dtype=torch.float32, device=dev).requires_grad_(want_fov)
    rs = sc.to(dev).settings()._replace(scale_modifier=cs.scale_modifier, antialiasing=antialiasing, return_alpha=dLa is not None,
                                        viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"],
                                        campos=leaves["campos"], tanfov=tf)
    out = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros_like(leaves["means3D"], requires_grad=True),
                                 opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                                 rotations=leaves["rotations"])
    val = (out[0] * dL.to(dev)).sum()
    if dLd is not None:
        val = val + (out[2] * dLd.to(dev)).sum()
    if dLa is not None:
        val = val + (out[3] * dLa.to(dev)).sum()
    val.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in leaves.items() if v.grad is not None}
    grads["tanfov"] = None if tf.grad is None else tf.grad.detach().cpu().numpy()
    grads["radii"] = out[1].cpu().numpy()
    return grads


@pytest.mark.parametrize("antialiasing", [False, True])
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("D", R.DEGREES)
@pytest.mark.parametrize("frame", R.FRAMES)
def test_dtanfov_matches_the_oracle(frame, D, loss, antialiasing):
    ref = R.oracle64(frame, D, loss, antialiasing)
    with_fov = _hip(frame, D, loss, antialiasing, True)
    without = _hip(frame, D, loss, antialiasing, False)
    assert without["tanfov"] is None and with_fov["tanfov"].shape == (2,)
    r = rel_l2(with_fov["tanfov"], ref["tanfov"])
    print(f"dtanfov {frame} D={D} {loss} aa={antialiasing}: rel-L2 {r:.3e}  got {with_fov['tanfov']}  want {ref['tanfov']}")
    assert r < R.BAR, (r, with_fov["tanfov"], ref["tanfov"])
    # requesting it changes no other gradient: on the whole frame to the order of the blend backward's float atomics
    # (`_one_quadrant`; 1e-6 is 25 × the 4e-8 two identical runs differ by) …
    assert set(with_fov) == set(without)
    for k in without:
        if k not in ("tanfov", "radii"):
            assert rel_l2(with_fov[k], without[k]) < 1e-6 or not without[k].any(), k
    # … and BIT FOR BIT where two backwards can be compared so: the same loss confined to one wave's pixels
    qa, qb = _hip(frame, D, loss, antialiasing, True, one_quadrant=True), _hip(frame, D, loss, antialiasing, False, one_quadrant=True)
    assert qb["tanfov"] is None and np.abs(qa["tanfov"]).max() > 0 and np.abs(qb["means3D"]).max() > 0
    for k in qb:
        if k != "tanfov":
            assert np.array_equal(qa[k], qb[k]), k
    for k in ("viewmatrix", "projmatrix"):   # (the sibling sums, for the record of what the bar is applied to)
        assert rel_l2(with_fov[k], ref[k]) < R.BAR, k


@pytest.mark.parametrize("frame", R.FRAMES)
def test_frozen_clamp_rows_contribute_what_the_oracle_says(frame):
    """The Gaussians beyond 1.3·tan(fov/2) carry a large part of dL/dtanfov (per Gaussian from the oracle, tan(fov/2) given as
    [P] tensors): a kernel that took the unclamped t.x / t.y for them, left them out, or differentiated the clamp's limit
    would miss the total by far more than the bar."""
    D, loss = 3, "colour"
    per = R.oracle_grads(frame, D, loss, False, per_gaussian=True)["tanfov"]          # [2,P]
    ref = R.oracle64(frame, D, loss, False)
    assert rel_l2(per.sum(1), ref["tanfov"]) < 1e-12
    cs = R.scene(frame, D)
    cls, _, _ = cs_.clamp_classes(cs, cs_.oracle_state(cs, use_sh=True))
    beyond = cls["x_only"] | cls["y_only"] | cls["both"]
    assert beyond.sum() >= 150
    share = per[:, beyond].sum(1)
    assert np.linalg.norm(share) > 0.25 * np.linalg.norm(ref["tanfov"])               # ≥ 125 × the bar
    # x-only rows beyond the clamp: J02 is frozen at the limit but still carries fx — a non-zero x term
    assert np.abs(per[0, cls["x_only"]]).max() > 0 and np.abs(per[1, cls["y_only"]]).max() > 0
    assert not per[:, ref["radii"] == 0].any()                                          # culled: nothing
    got = _hip(frame, D, loss, False, True)
    assert np.array_equal(got["radii"], ref["radii"])
    assert rel_l2(got["tanfov"], ref["tanfov"]) < R.BAR


# ---- launch sets and Gaussian sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V", [(1, 3), (2, 4)])
def test_dtanfov_of_launch_sets_and_gaussian_sets(B, V):
    """Each view's dL/dtanfov row of a launch set (V = 3 views of one set; B = 2 sets × 2 views) equals the single-view call's to
    the fp32 summation-order difference tests/test_gpu_views_batched.py allows the sibling dL/dviewmatrix (rel-L2 2e-6), and is
    bit-identical across two runs (of a loss whose blend backward is order-free, see `_one_quadrant`).  The views are those of
    tests/tanfov_reference.py `LS_VIEWS`: cameras and upstream gradients whose sums do not cancel (A < 4, measured on the oracle),
    since the order of the blend backward's float atomics, which the two calls do not share, is magnified by the cancellation."""
    from ggrt_official_amd import GaussianRasterizer
    from ggrt_official_amd.rasterizer import rasterize_views
    (W, H), P = R.LS_FRAME, R.LS_P
    vps = V // B
    views = R.LS_VIEWS[(B, V)]
    assert len(views) == V and [s for s, _c, _u in views] == [v // vps for v in range(V)]
    scs = [R.ls_scene(b) for b in range(B)]
    cams = [R.ls_camera(s, cam) for s, cam, _u in views]
    view, full, campos = (torch.stack([c[i] for c in cams]).float().to(dev) for i in range(3))
    tanfov = torch.tensor([[c[3], c[4]] for c in cams], dtype=torch.float32, device=dev)
    dLs = torch.stack([R.ls_upstream(up)[0] for _s, _c, up in views]).to(dev)
    dDs = torch.stack([R.ls_upstream(up)[1] for _s, _c, up in views]).to(dev)
    bgs = R.ls_backgrounds(V).to(dev)
    stack = lambda f: (torch.stack([f(s) for s in scs]) if B > 1 else f(scs[0])).to(dev)
    inputs = dict(means3D=stack(lambda s: s.means3D), opacities=stack(lambda s: s.opacities), shs=stack(lambda s: s.shs),
                  scales=stack(lambda s: s.scales), rotations=stack(lambda s: s.rotations))
    rs = scs[0].to(dev).settings()

    def run_set(gc, gd):
        lv = {k: _leaf(t) for k, t in inputs.items()}
        cams = [_leaf(view), _leaf(full), _leaf(campos)]
        tf = _leaf(tanfov)
        m, o = lv.pop("means3D"), lv.pop("opacities")
        color, radii, depth = rasterize_views(m, o, *cams, bgs, tf, rs, **lv)
        ((color * gc).sum() + (depth * gd).sum()).backward()
        torch.cuda.synchronize()
        return tf.grad.cpu().numpy(), cams[0].grad.cpu().numpy(), m.grad.cpu().numpy()

    a, va, ma = run_set(dLs, dDs)
    # bit-identical across two runs: the partial sums are reduced in a fixed order, without atomics — asked where the blend
    # backward's records in front of them are order-free as well (`_one_quadrant`)
    q1, q2 = run_set(_one_quadrant(dLs), _one_quadrant(dDs)), run_set(_one_quadrant(dLs), _one_quadrant(dDs))
    assert a.shape == (V, 2) and np.abs(q1[0]).min() > 0
    for x, y in zip(q1, q2):
        assert np.array_equal(x, y)
    for v in range(V):
        s = v // vps
        pick = (lambda t: t[s]) if B > 1 else (lambda t: t)
        lv = {k: _leaf(pick(t)) for k, t in inputs.items()}
        tf = _leaf(tanfov[v])
        cams = [_leaf(view[v]), _leaf(full[v]), _leaf(campos[v])]
        one = rs._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2], bg=bgs[v], tanfov=tf)
        color, radii, depth = GaussianRasterizer(one)(means3D=lv["means3D"], means2D=torch.zeros_like(lv["means3D"]),
                                                      opacities=lv["opacities"], shs=lv["shs"], scales=lv["scales"],
                                                      rotations=lv["rotations"])
        ((color * dLs[v]).sum() + (depth * dDs[v]).sum()).backward()
        torch.cuda.synchronize()
        r = rel_l2(a[v], tf.grad.cpu().numpy())
        print(f"sets B={B} V={V} view {v}: dtanfov {a[v]} single {tf.grad.cpu().numpy()} rel-L2 {r:.2e}")
        assert np.abs(a[v]).min() > 0
        assert r < 2e-6, (v, r)
        assert rel_l2(va[v], cams[0].grad.cpu().numpy()) < 2e-6


# ---- camera_setup backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_invariant", [True, False])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_camera_setup_backward_matches_float64_autograd(n, scale_invariant):
    from ggrt_official_amd.rasterizer import camera_setup
    ext, intr, near, far = cr.cameras(n, seed=n)
    g = torch.Generator().manual_seed(100 + n)
    ups = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((n, 4, 4), (n, 4, 4), (n, 3), (n, 2))]

    def reference(mask):
        e, k = ext.double().requires_grad_(), intr.double().requires_grad_()
        outs = cr.camera_setup_ref(e, k, near, far, scale_invariant)
        sum((o * u).sum() * m for o, u, m in zip(outs[:4], ups, mask)).backward()
        return [o.detach().numpy() for o in outs], e.grad.numpy(), k.grad.numpy()

    def device(mask):
        e, k = _leaf(ext), _leaf(intr)
        outs = camera_setup(e, k, near.to(dev), far.to(dev), scale_invariant)
        assert not outs[4].requires_grad
        sum((o * u.float().to(dev)).sum() * m for o, u, m in zip(outs[:4], ups, mask)).backward()
        torch.cuda.synchronize()
        return [o.detach().cpu().numpy() for o in outs], e.grad.cpu().numpy(), k.grad.cpu().numpy()

    outs_r, dE_r, dK_r = reference((1, 1, 1, 1))
    outs_d, dE_d, dK_d = device((1, 1, 1, 1))
    fwd_err = max(rel_l2(d, r) for d, r in zip(outs_d[:4], outs_r[:4]))
    bar = 4.0 * fwd_err
    eE, eK = rel_l2(dE_d, dE_r), rel_l2(dK_d, dK_r)
    print(f"camera_setup n={n} scale_invariant={scale_invariant}: forward rel-L2 {fwd_err:.3e}, bar {bar:.3e}, "
          f"dL/dextrinsics {eE:.3e}, dL/dintrinsics {eK:.3e}")
    assert 1e-9 < fwd_err < 1e-6
    assert eE < bar and eK < bar, (eE, eK, bar)
    # bit-reproducible (the sum into row 0 has a fixed order)
    _, dE_2, dK_2 = device((1, 1, 1, 1))
    assert np.array_equal(dE_d, dE_2) and np.array_equal(dK_d, dK_2)
    # the structure: without a tan(fov/2) gradient only row 0 is written — the projection terms of ALL n views …
    _, _, dK_proj_r = reference((1, 1, 1, 0))
    _, _, dK_proj = device((1, 1, 1, 0))
    assert not dK_proj[1:].any() and not dK_proj_r[1:].any()
    assert rel_l2(dK_proj[0], dK_proj_r[0]) < bar
    if n > 1:   # (… not view 0's alone)
        ext1, intr1 = ext[:1], intr[:1]
        e1, k1 = ext1.double().requires_grad_(), intr1.double().requires_grad_()
        o1 = cr.camera_setup_ref(e1, k1, near[:1], far[:1], scale_invariant)
        sum((o * u[:1]).sum() for o, u in zip(o1[:3], ups[:3])).backward()
        assert rel_l2(dK_proj[0], k1.grad[0].numpy()) > 0.05
    # … and with it alone every row holds its own view's fov terms, row 0 nothing else
    _, dE_fov_r, dK_fov_r = reference((0, 0, 0, 1))
    _, dE_fov, dK_fov = device((0, 0, 0, 1))
    assert not dE_fov.any()
    for i in range(n):
        assert np.abs(dK_fov[i]).max() > 0 and rel_l2(dK_fov[i], dK_fov_r[i]) < bar, i
    # rows >= 1 of the whole gradient are the fov terms alone, bit for bit; row 0 is the two parts' sum
    assert np.array_equal(dK_d[1:], dK_fov[1:])
    assert rel_l2(dK_d[0], dK_proj_r[0] + dK_fov_r[0]) < bar


def test_camera_setup_forward_is_unchanged_and_singular_pose_gives_nan():
    from ggrt_official_amd.rasterizer import camera_setup
    ext, intr, near, far = cr.cameras(3, seed=8)
    plain = camera_setup(ext.to(dev), intr.to(dev), near.to(dev), far.to(dev), True)
    e, k = _leaf(ext), _leaf(intr)
    grad = camera_setup(e, k, near.to(dev), far.to(dev), True)
    for a, b in zip(plain, grad):
        assert torch.equal(a, b)
    assert not any(t.requires_grad for t in plain) and all(t.requires_grad for t in grad[:4])
    bad = ext.clone()
    bad[1] = 0.0                                          # singular: the forward writes NaN for this view
    e = _leaf(bad)
    outs = camera_setup(e, k, near.to(dev), far.to(dev), True)
    sum(o.sum() for o in outs[:4]).backward()
    torch.cuda.synchronize()
    assert torch.isnan(e.grad[1]).all() and torch.isfinite(e.grad[0]).all() and torch.isfinite(e.grad[2]).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _call_site_case(v=2, P=2000, W=64, H=48, D=1):
    """One batch element seen by `v` cameras near the scene's own: (Gaussians as the decoder gets them, extrinsics, intrinsics,
    near, far, dL [v,3,H,W], the scene)"""
    from ggrt_official_amd import splatting as sp
    c2w = cs_.pose(3).float()
    sc = make_scene(P, W, H, sh_degree=D, profile="A", seed=4, c2w=c2w)
    ext = torch.stack([(c2w.double() @ cs_.pose(40 + i, angle=0.08, shift=0.1)).float() if i else c2w for i in range(v)])
    intr = torch.eye(3).repeat(v, 1, 1)
    for i in range(v):
        intr[i, 0, 0], intr[i, 1, 1] = 0.5 / sc.tanfovx * (1 + 0.04 * i), 0.5 / sc.tanfovy * (1 - 0.03 * i)
        intr[i, 0, 2], intr[i, 1, 2] = 0.5 + 0.03 * (i + 1), 0.5 - 0.02 * (i + 1)
    near, far = torch.tensor([0.9 + 0.05 * i for i in range(v)]), torch.full((v,), 80.0)
    cov33 = sc.cov3D[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    gs = sp.Gaussians(means=sc.means3D[None].to(dev), covariances=cov33[None].to(dev),
                      harmonics=sc.shs.permute(0, 2, 1)[None].contiguous().to(dev), opacities=sc.opacities[None, :, 0].to(dev))
    dL = torch.stack([upstream_gradient(W, H, seed=30 + i) for i in range(v)])
    return gs, ext, intr, near, far, dL, sc


def _call_site_reference(ext, intr, near, far, dL, sc, fov_gradient=True):
    """The whole chain in float64: tests/camera_reference.py in front of the torch oracle, tan(fov/2) as tensors —
    `fov_gradient=False` detaches them (what the call site returned while tan(fov/2) went through the host)."""
    e, k = ext.double().requires_grad_(), intr.double().requires_grad_()
    view, full, campos, tanfov, scale = cr.camera_setup_ref(e, k, near, far, True)
    if not fov_gradient:
        tanfov = tanfov.detach()
    loss = 0.0
    for i in range(ext.shape[0]):
        color, _, _ = tr.rasterize(sc.means3D.double() * scale[i], sc.opacities.double(), view[i], full[i], campos[i], sc.bg,
                                   sc.width, sc.height, tanfov[i, 0], tanfov[i, 1], sc.sh_degree, shs=sc.shs.double(),
                                   cov3D_precomp=sc.cov3D.double() * scale[i] ** 2, sh_cap=3)
        loss = loss + (color * dL[i].double()).sum()
    loss.backward()
    return e.grad.numpy(), k.grad.numpy()


def test_call_site_pose_and_intrinsics_gradients_end_to_end():
    """`render_views_fused` (DecoderSplattingCUDA's path) with GPU extrinsics / intrinsics that require grad stays on the
    device path and returns the WHOLE intrinsics gradient — the part through the splat footprints (tan(fov/2)) included, which
    the call site dropped while tan(fov/2) travelled as host floats."""
    from ggrt_official_amd import splatting as sp
    gs, ext, intr, near, far, dL, sc = _call_site_case()
    v, H, W = ext.shape[0], sc.height, sc.width

    def run(device_camera):
        e, k = _leaf(ext), _leaf(intr)
        color, _ = sp.render_views_fused(e, k, near.to(dev), far.to(dev), (H, W), sc.bg.to(dev)[None].expand(v, 3), gs,
                                         [0] * v, None, device_camera=device_camera, sh_max_degree=3)
        (color * dL.to(dev)).sum().backward()
        torch.cuda.synchronize()
        return color.detach().cpu().numpy(), e.grad.cpu().numpy(), k.grad.cpu().numpy()

    col_d, dE_d, dK_d = run(True)
    col_t, dE_t, dK_t = run(False)
    dE_ref, dK_ref = _call_site_reference(ext, intr, near, far, dL, sc)
    _, dK_partial = _call_site_reference(ext, intr, near, far, dL, sc, fov_gradient=False)
    figs = dict(ext_vs_torch_branch=rel_l2(dE_d, dE_t), ext_vs_reference=rel_l2(dE_d, dE_ref), intr_vs_reference=rel_l2(dK_d, dK_ref),
                intr_torch_branch_vs_reference=rel_l2(dK_t, dK_ref), intr_vs_projection_part_only=rel_l2(dK_d, dK_partial))
    print("call site:", {a: f"{b:.3e}" for a, b in figs.items()})
    assert np.abs(col_d - col_t).max() < 2e-3
    assert figs["ext_vs_torch_branch"] < 2e-3 and figs["ext_vs_reference"] < 2e-3
    assert figs["intr_vs_reference"] < 2e-3
    assert figs["intr_torch_branch_vs_reference"] < 2e-3           # both branches give the whole gradient
    assert figs["intr_vs_projection_part_only"] > 10 * 2e-3         # … which the projection part alone is far from
    assert np.abs(dK_d[1:]).max() > 0                                # rows >= 1: their views' fov terms (zero before)


def test_decoder_keeps_poses_with_gradients_on_the_device_path(monkeypatch):
    """DecoderSplattingCUDA with extrinsics / intrinsics that require grad: camera_setup runs (no torch formulation, no
    device-to-host copy of tan(fov/2)), and both receive gradients."""
    from ggrt_official_amd import rasterizer, splatting as sp
    gs, ext, intr, near, far, dL, sc = _call_site_case()
    calls = []
    real = rasterizer.camera_setup
    monkeypatch.setattr(rasterizer, "camera_setup", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    monkeypatch.setattr(sp, "get_fov", lambda *_a, **_k: (_ for _ in ()).throw(AssertionError("the torch branch ran")))
    e, k = _leaf(ext[None]), _leaf(intr[None])
    out = sp.DecoderSplattingCUDA(sh_max_degree=3).to(dev)(gs, e, k, near[None].to(dev), far[None].to(dev), (sc.height, sc.width))
    (out.color[0] * dL.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert calls == [1]
    assert torch.isfinite(e.grad).all() and torch.isfinite(k.grad).all() and k.grad[0, 1].abs().max() > 0


# ---- sync-free -------------------------------------------------------------------------------------------------------------------
def test_pose_gradient_step_replays_from_a_hip_graph():
    """The pose-gradient training step (forward + backward to extrinsics.grad / intrinsics.grad) captured with
    torch.cuda.graph in the setup of tests/test_gpu_sync_free.py, replayed twice with changed poses: each replay equals its
    eager exact-mode result (colour bit for bit, gradients to that test's 1e-5)."""
    from ggrt_official_amd import splatting as sp
    gs, ext, intr, near, far, dL, sc = _call_site_case(v=1)
    H, W = sc.height, sc.width
    nr, fr, bg, dLd = near.to(dev), far.to(dev), sc.bg.to(dev)[None], dL.to(dev)
    e, k = _leaf(ext), _leaf(intr)

    def step(e, k, capacity):
        e.grad = k.grad = None
        color, _ = sp.render_views_fused(e, k, nr, fr, (H, W), bg, gs, [0], None, list_capacity=capacity, sh_max_degree=3)
        color.backward(dLd)
        return color

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(e, k, 400_000)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_color = step(e, k, 400_000)
    g_e, g_k = e.grad, k.grad
    for r in range(2):
        with torch.no_grad():
            e.copy_((ext.double() @ cs_.pose(90 + r, angle=0.05, shift=0.08)).float().to(dev))
            k[:, 0, 2] += 0.01
        graph.replay()
        torch.cuda.synchronize()
        got = [g_color.clone(), g_e.clone(), g_k.clone()]
        e2, k2 = _leaf(e), _leaf(k)
        color = step(e2, k2, 0)
        torch.cuda.synchronize()
        assert torch.equal(got[0], color.detach())
        assert rel_l2(got[1].cpu().numpy(), e2.grad.cpu().numpy()) < 1e-5
        assert rel_l2(got[2].cpu().numpy(), k2.grad.cpu().numpy()) < 1e-5
        assert got[2][0].abs().max() > 0
