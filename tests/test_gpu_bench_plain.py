"""bench.py's plain run (`-m gpu`): without `--full` it times exactly the K steps it is given and prints the headline only;
`--dump-outputs DIR` leaves what the last timed step returned, in float32, within the 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "C2",
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["unit"] == "Mpix/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["value"] > 0
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["step_ms_hip_events"]["n"] == 3
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(504 * 378 / rec["ms_per_step"] / 1e3, rel=2e-3)
    for k in ("stages_ms", "roofline", "secondary", "cpu_baseline", "hipgraph_replay", "list_hint"):
        assert k not in rec, k                        # the informational legs run with --full only
    arrays = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"color", "depth", "radii", "grad_means3D", "grad_shs", "grad_opacities", "grad_viewmatrix"} <= set(arrays)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["color"].shape == (3, 378, 504) and arrays["color"].max() > 0
    assert arrays["radii"].shape == (65_536,) and (arrays["radii"] > 0).any() and np.abs(arrays["grad_shs"]).max() > 0
