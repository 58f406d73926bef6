"""The absgrad pass driven from plain C (`tests/c_abi/absgrad_smoke.c`, gcc, C11): the header's additions are valid C, the library
links, and (on the GPU) a training forward + ggr_means2d_absgrad give absgrad >= |grad| with the cancellation a sign-alternating
gradient must show, exact zeros for a Gaussian moved off screen, and the documented return codes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "absgrad_smoke.c")
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


def test_absgrad_host_compiles_and_links_from_c(tmp_path):
    assert os.path.getsize(_build(str(tmp_path / "absgrad_smoke"))) > 0


@pytest.mark.gpu
def test_c_host_absgrad_known_properties(tmp_path):
    exe = _build(str(tmp_path / "absgrad_smoke"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ABSGRAD C ABI SMOKE OK" in r.stdout, r.stdout
