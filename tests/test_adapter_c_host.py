"""The Gaussian adapter pass driven from plain C (`tests/c_abi/adapter_smoke.c`, gcc, C11): the header's additions are valid C, the
library links, every invalid pass is refused before anything is enqueued, and (on the GPU) forward and backward reproduce the
closed forms of an identity camera that the C host checks itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "adapter_smoke.c")
LIBDIR = os.path.join(ROOT, "ggrt_official_amd")


def _build(out):
    from ggrt_official_amd import _build
    _build.build_library()
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-D__HIP_PLATFORM_AMD__", SRC,
           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-L" + LIBDIR, "-L/opt/rocm/lib", "-lggr_raster",
           "-lamdhip64", "-lm", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def test_adapter_host_compiles_and_links_from_c(tmp_path):
    assert os.path.getsize(_build(str(tmp_path / "adapter_smoke"))) > 0


@pytest.mark.gpu
def test_c_host_adapter_reproduces_the_closed_forms(tmp_path):
    exe = _build(str(tmp_path / "adapter_smoke"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ADAPTER C ABI SMOKE OK" in r.stdout, r.stdout
