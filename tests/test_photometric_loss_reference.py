"""tests/photometric_loss_reference.py against the reference's own `MultiViewPhotometricDecayLoss` (tests/golden/
photometric_loss_*.npz, written by tests/golden/make_photometric_loss_golden.py from the reference's modules): the restatement in
float64 reproduces the float64 fixtures to about 1e-10 relative, and in float32 it is as close to them as the reference's own
float32 run is (4 x that distance, floor 1e-6: two float32 runs of the same arithmetic in another order).  Then the conditions the
GPU test puts on its inputs, checked here in float32 against float64 before any GPU time is spent: at most 3 % of a case's
pixel-iterations undecided, float32 making float64's decisions on the decided ones, and every case with warped winners, unwarped
winners, clamped pixels and out-of-frame samples."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.photometric_loss_reference import DEFAULTS, decided_pixels, make_photometric_case, run_photometric_loss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(f)[len("photometric_loss_"):-len(".npz")] for f in glob.glob(os.path.join(GOLDEN, "photometric_loss_*.npz")))
KEYS = ("loss", "photometric_loss", "smoothness_loss", "g_inv_depths", "g_poses")


def _load(name):
    z = np.load(os.path.join(GOLDEN, f"photometric_loss_{name}.npz"), allow_pickle=False)
    case = {k: torch.from_numpy(z[k]) for k in ("image", "ref_imgs", "inv_depths", "K", "ref_Ks", "poses")}
    opts = {k[4:]: (bool(z[k]) if k == "opt_automask_loss" else float(z[k])) for k in z.files if k.startswith("opt_")}
    return z, case, opts


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_fixtures_are_there_and_small():
    assert NAMES == ["v1n1_tiny", "v2n3_default", "v3n2_noclip_nomask"]
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"photometric_loss_{name}.npz")) < 96 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_in_float64_reproduces_the_reference(name):
    z, case, opts = _load(name)
    got = run_photometric_loss("torch", case, torch.float64, "cpu", **opts)
    for k in KEYS:
        e = _rel(got[k].numpy().reshape(z[k + "64"].shape), z[k + "64"]) if np.abs(z[k + "64"]).max() > 0 else float(got[k].abs().max())
        print(f"{name} {k}: relative error {e:.3e}")
        assert e <= 1e-10, (name, k, e)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_in_float32_is_as_close_as_the_reference_in_float32(name):
    z, case, opts = _load(name)
    got = run_photometric_loss("torch", case, torch.float32, "cpu", **opts)
    for k in KEYS:
        if np.abs(z[k + "64"]).max() == 0:
            assert float(got[k].abs().max()) == 0
            continue
        own = _rel(z[k + "32"], z[k + "64"])
        e = _rel(got[k].numpy().reshape(z[k + "64"].shape), z[k + "64"])
        print(f"{name} {k}: restatement {e:.3e}, the reference's own float32 {own:.3e}")
        assert e <= max(4 * own, 1e-6), (name, k, e, own)


def test_decisions_override_reproduces_the_free_run():
    case = make_photometric_case(2, 2, 17, 33, 11)
    a = run_photometric_loss("torch", case, torch.float64, "cpu")
    b = run_photometric_loss("torch", case, torch.float64, "cpu", decisions=(a["choice"], a["unclamped"]))
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


# the cases of tests/test_gpu_photometric_loss.py (imported there): name -> (V, n, H, W, seed, options)
GPU_CASES = {
    "h2": (1, 1, 2, 40, 21, {}), "h15": (1, 2, 15, 20, 22, {}), "h16": (2, 1, 16, 20, 23, {}), "h17": (1, 1, 17, 20, 24, {}),
    "h33": (1, 1, 33, 12, 25, {}), "w2": (1, 1, 24, 2, 26, {}), "w31": (1, 1, 9, 31, 27, {}), "w32": (2, 2, 9, 32, 28, {}),
    "w33": (1, 1, 9, 33, 29, {}), "w65": (1, 1, 9, 65, 30, {}), "both": (2, 2, 17, 33, 31, {}),
    "v5": (5, 2, 17, 33, 32, {}), "n13": (2, 13, 17, 33, 33, {}),
    "nomask": (2, 2, 17, 33, 34, dict(automask_loss=False)), "noclip": (2, 2, 17, 33, 35, dict(clip_loss=0.0)),
    "nosmooth": (2, 2, 17, 33, 36, dict(smooth_loss_weight=0.0)),
}


def input_conditions(name):
    V, n, H, W, seed, opts = GPU_CASES[name]
    case = make_photometric_case(V, n, H, W, seed)
    ref = run_photometric_loss("torch", case, torch.float64, "cpu", **opts)
    t32 = run_photometric_loss("torch", case, torch.float32, "cpu", **opts)
    delta = 8 * float((t32["planes"].double() - ref["planes"]).abs().max())
    clip = opts.get("clip_loss", DEFAULTS["clip_loss"])
    decided = decided_pixels(ref, delta, clip)
    undecided = 1.0 - float(decided.double().mean())
    agree = bool((t32["choice"] == ref["choice"])[decided].all() and (t32["unclamped"] == ref["unclamped"])[decided].all())
    H_, W_ = ref["planes"].shape[-2:]
    u, v = ref["coords"][:, :, 0], ref["coords"][:, :, 1]
    automask = opts.get("automask_loss", True)
    facts = dict(undecided=undecided, delta=delta, agree=agree,
                 warped_winners=int(((ref["choice"] % 2 == 0) if automask else torch.ones_like(ref["choice"], dtype=torch.bool)).sum()),
                 unwarped_winners=int((ref["choice"] % 2 == 1).sum()) if automask else None,
                 clamped=int((~ref["unclamped"]).sum()) if clip > 0 else None,
                 out_of_frame=int(((u < 0) | (u > W_ - 1) | (v < 0) | (v > H_ - 1)).sum()))
    return facts


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_the_gpu_cases_meet_their_input_conditions_in_float32_on_the_cpu(name):
    f = input_conditions(name)
    print(f"{name}: {f}")
    assert f["undecided"] <= 0.03, f
    assert f["agree"], f
    assert f["warped_winners"] > 0 and f["out_of_frame"] > 0, f
    assert f["unwarped_winners"] is None or f["unwarped_winners"] > 0, f
    assert f["clamped"] is None or f["clamped"] > 0, f
