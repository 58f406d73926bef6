"""The encoded epipolar-attention pass driven from plain C (`tests/c_abi/epipolar_attn_enc_smoke.c`, gcc, C11): the header's
additions are valid C, the library links, and — in a process without a GPU — the struct has the documented layout, invalid passes
are refused before anything is enqueued and the empty call succeeds with every pointer NULL.  On the GPU the same host runs
forward and backward where the answer is known in closed form: qk = qe = 0 gives uniform weights, and depths of 0, 1/4 and 1/2
put the sines of both octaves at 0 and ±1, so ctx_e, dL/dqe and dL/ddepth are small rationals (times F)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "epipolar_attn_enc_smoke.c")
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


def test_encoded_attention_host_links_from_c_and_refuses_invalid_passes_without_a_gpu(tmp_path):
    exe = _build(str(tmp_path / "epipolar_attn_enc_smoke"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # (no GPU for this process, wherever it runs)
    r = subprocess.run([exe, "--host-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "ENCODED EPIPOLAR ATTENTION C ABI HOST CHECKS OK" in r.stdout, r.stdout


@pytest.mark.gpu
def test_c_host_encoded_attention_reproduces_the_closed_forms(tmp_path):
    exe = _build(str(tmp_path / "epipolar_attn_enc_smoke"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ENCODED EPIPOLAR ATTENTION C ABI SMOKE OK" in r.stdout, r.stdout
