"""Whole-log RTS smoothing of 64 independent log segments of different lengths as ONE batch (SegmentBatcher::enableSmoothing / smooth,
tests/cpp/test_segments_smooth.cpp): every segment's smoothed posteriors against a single-segment run of its log through the two-argument
EKFSmoothBackwardsPass and, for four of them, against the oracle's recursion; equal-length logs bit for bit the two-argument pass without
a select launch; after a segment's end its rows carry its final posterior bit for bit, where the two-argument pass leaves the idle state
(which differs from it only at rounding level on these logs; the two passes' emitted rows agree to rounding and are only printed).  The
lead segment changes mid-run."""
import os
import subprocess

import pytest

from pronto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARG = {15: [], 21: ["n21"]}  # tests/cpp/test_n.hpp


def build_exe(oracle, name):
    _lib.build()
    exe = os.path.join(ROOT, "tests", "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "test_n.hpp"), os.path.join(ROOT, "pronto_amd", "csrc", "mav_state_est_batch.hpp"),
            os.path.join(ROOT, "pronto_amd", "csrc", "mav_state_est.hpp"), os.path.join(ROOT, "pronto_amd", "csrc", "segment_batcher.hpp"), os.path.join(ROOT, "pronto_amd", "csrc", "segment_stream.hpp"),
            os.path.join(ROOT, "pronto_amd", "csrc", "segment_channels.hpp"),
            os.path.join(ROOT, "pronto_amd", "csrc", "lcm_schema.hpp"),
            os.path.join(ROOT, "pronto_amd", "csrc", "pronto_wire.hpp"),
            os.path.join(ROOT, "include", "pronto_batch.h"), _lib.LIB_PATH]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    cmd = ["g++", "-O1", "-std=c++17", "-fopenmp", "-Wall", "-Werror=return-type", "-o", exe, src,
           "-L" + os.path.dirname(_lib.LIB_PATH), "-lpronto_batch", "-L" + os.path.join(ROOT, "oracle", "build"),
           "-lpronto_oracle", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("every", [1, 5])
def test_smoothing_independent_log_segments_of_different_lengths_on_gpu(oracle, tmp_path, n, fuse, every):
    exe = build_exe(oracle, "test_segments_smooth")
    args = [exe, str(tmp_path), "every=%d" % every] + ([] if fuse else ["nofuse"]) + NARG[n]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
