"""The ConvGRU inference route driven from plain C (`tests/c_abi/gru_conv_smoke.c`, gcc, C11): the header's additions are valid C,
the library links, and — in a process without a GPU — the struct has the documented size and invalid passes are refused before
anything is enqueued.  On the GPU the same host runs one GATE and one BLEND (and the RAW sums of both) with 1 x 5 and 3 x 3 kernels
against values it computes itself in double."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "gru_conv_smoke.c")
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


def test_gru_conv_host_links_from_c_and_refuses_invalid_passes_without_a_gpu(tmp_path):
    exe = _build(str(tmp_path / "gru_conv_smoke"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # (no GPU for this process, wherever it runs)
    r = subprocess.run([exe, "--host-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "GRU CONV C ABI HOST CHECKS OK" in r.stdout, r.stdout


@pytest.mark.gpu
def test_c_host_gru_conv_reproduces_the_host_values(tmp_path):
    exe = _build(str(tmp_path / "gru_conv_smoke"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "GRU CONV C ABI SMOKE OK" in r.stdout, r.stdout
