"""What LaserGPFHandler, GridLikelihood and RBISGPFMeasurement (pronto_amd/csrc/mav_state_est_gpf.hpp) ask the device to do, recorded on
the CPU: tests/cpp/gpf_trace.cpp runs named scenarios against the recording C ABI -- the unchanged tests/cpp/abi_recorder.cpp and
abi_recorder_wide.cpp plus tests/cpp/abi_recorder_gpf.cpp, which defines the pb_gpf_* family alone -- and each scenario's output must
equal tests/golden/gpf_trace/<scenario>.txt byte for byte, for the plain build and for one with -fsanitize=address,undefined.  Every
substate list, a scan with points per filter, an update re-applied after a late arrival (the same stream_id twice), a bad substate
(the reference's fatal error: exit code 1) and gpf_num_samples = 0."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pronto_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gpf_trace")
SCENARIOS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
LISTS = {"pos_only": "[9,10,11]", "pos_yaw": "[8,9,10,11]", "pos_chi": "[6,7,8,9,10,11]", "all_states": "[3,4,5,6,7,8,9,10,11]", "z_only": "[11]"}


def build_exe(build):
    exe = os.path.join(ROOT, "tests", "build", "gpf_trace_" + build)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    header = os.path.join(CSRC, "mav_state_est_gpf.hpp")
    srcs = [os.path.join(ROOT, "tests", "cpp", f) for f in ("gpf_trace.cpp", "abi_recorder.cpp", "abi_recorder_wide.cpp", "abi_recorder_gpf.cpp")]
    deps = srcs + [header] + [os.path.join(CSRC, h) for h in ("mav_state_est_wide.hpp", "mav_state_est_batch.hpp", "mav_state_est.hpp")] + [
        os.path.join(ROOT, "tests", "cpp", "abi_recorder.h"), os.path.join(ROOT, "include", "pronto_batch.h")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", '-DSHIM_HEADER="%s"' % header] + BUILDS[build]
                          + ["-o", exe] + srcs)
    return exe


def test_every_scenario_has_a_golden_trace():
    listed = subprocess.run([build_exe("plain"), "--list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(listed) == SCENARIOS and len(SCENARIOS) == 9


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_gpf_trace_equals_golden(scenario, build):
    r = subprocess.run([build_exe(build), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    with open(os.path.join(GOLDEN, scenario + ".txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got, exp = r.stdout.decode(errors="replace").splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        pytest.fail("%s (%s): trace differs from line %d\n  got:    %s\n  golden: %s" % (
            scenario, build, first + 1, "\n          ".join(got[first:first + 8]), "\n          ".join(exp[first:first + 8])))
    assert r.returncode == (1 if scenario == "bad_substate" else 0)


def test_goldens_say_what_the_issue_asks():
    """read from the goldens themselves: the substate lists, the replayed stream ids, the refusals"""
    text = {s: open(os.path.join(GOLDEN, s + ".txt")).read() for s in SCENARIOS}
    for s, idx in LISTS.items():
        calls = [ln for ln in text[s].splitlines() if ln.startswith(("pb_gpf_sample", "pb_gpf_measurement", "pb_update_indexed_wide"))]
        assert len(calls) == 6 and all("idx=%s " % idx in ln for ln in calls), s
        assert "cov_scaling=2.25" in text[s] and text[s].count("pb_gpf_grid_set") == 1
    ids = [int(v) for v in re.findall(r"pb_gpf_normals seed=42 stream_id=(\d+)", text["late_scan"])]
    assert sorted(set(ids)) == [0, 1] and ids.count(0) >= 2 and ids.count(1) >= 2, ids
    assert "pb_" not in text["bad_substate"] and "unknown gpf_substate 'pos_and_velocity'" in text["bad_substate"]
    assert "pb_gpf" not in text["zero_samples"] and "-> NULL" in text["zero_samples"]
