"""The opt-in shim header pronto_amd/csrc/mav_state_est_gpf.hpp on the GPU: tests/cpp/test_gpf_update.cpp replays a written log with two
laser scans through LogPlayer + LaserGPFHandler + GridLikelihood into 70 filters with posterior checkpoints, in order and with the
first scan delivered late.  The two heads must be equal value for value: a re-applied RBISGPFMeasurement draws the same normals (its
stream_id is its serial number)."""
import os
import subprocess

import pytest

from pronto_amd import _lib
from test_cpp_shim import NARG, ROOT


def build_exe():
    _lib.build()
    exe = os.path.join(ROOT, "tests", "build", "test_gpf_update")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_gpf_update.cpp")
    csrc = os.path.join(ROOT, "pronto_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "test_n.hpp"), os.path.join(ROOT, "include", "pronto_batch.h"), _lib.LIB_PATH] + [
        os.path.join(csrc, h) for h in ("mav_state_est_gpf.hpp", "mav_state_est_wide.hpp", "mav_state_est_batch.hpp", "mav_state_est.hpp",
                                        "lcm_schema.hpp", "pronto_wire.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-Wall", "-Werror=return-type", "-o", exe, src,
                           "-L" + os.path.dirname(_lib.LIB_PATH), "-lpronto_batch", "-L" + os.path.join(ROOT, "oracle", "build"),
                           "-lpronto_oracle", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_gpf_shim_links_without_a_gpu(oracle):
    """the header compiles and links against the library everywhere"""
    assert os.path.exists(build_exe())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
def test_two_scans_in_order_and_late_on_gpu(oracle, tmp_path, n):
    r = subprocess.run([build_exe(), str(tmp_path)] + NARG[n], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
