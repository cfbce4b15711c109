"""The opt-in shim header pronto_amd/csrc/mav_state_est_flow.hpp: tests/cpp/test_flow_update.cpp replays a written log with two
pronto::optical_flow_t messages through LogPlayer + OpticalFlowHandler into 70 filters with posterior checkpoints, in order and with
the first message delivered late.  The two heads must be equal value for value: a re-applied RBISOpticalFlowMeasurement owns its
message.  Without a GPU: the header compiles and links, and the two base headers still do not name the pb_flow functions."""
import os
import re
import subprocess

import pytest

from pronto_amd import _lib
from test_cpp_shim import NARG, ROOT

CSRC = os.path.join(ROOT, "pronto_amd", "csrc")


def build_exe():
    _lib.build()
    exe = os.path.join(ROOT, "tests", "build", "test_flow_update")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_flow_update.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "test_n.hpp"), os.path.join(ROOT, "include", "pronto_batch.h"), _lib.LIB_PATH] + [
        os.path.join(CSRC, h) for h in ("mav_state_est_flow.hpp", "mav_state_est_batch.hpp", "mav_state_est.hpp", "lcm_schema.hpp", "pronto_wire.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-Wall", "-Werror=return-type", "-o", exe, src,
                           "-L" + os.path.dirname(_lib.LIB_PATH), "-lpronto_batch", "-L" + os.path.join(ROOT, "oracle", "build"),
                           "-lpronto_oracle", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_flow_shim_links_without_a_gpu(oracle):
    """the header compiles and links against the library everywhere"""
    assert os.path.exists(build_exe())


def test_base_headers_do_not_name_the_flow_entry_points():
    for h in ("mav_state_est.hpp", "mav_state_est_batch.hpp", "mav_state_est_wide.hpp", "mav_state_est_gpf.hpp"):
        assert not re.search(r"pb_flow_set_camera|pb_update_optical_flow", open(os.path.join(CSRC, h)).read()), h
    assert "pb_update_optical_flow" in open(os.path.join(CSRC, "mav_state_est_flow.hpp")).read()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
def test_two_flow_messages_in_order_and_late_on_gpu(oracle, tmp_path, n):
    r = subprocess.run([build_exe(), str(tmp_path)] + NARG[n], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
