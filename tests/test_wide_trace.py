"""What WideIndexedMeasurementHandler and the wide update classes (pronto_amd/csrc/mav_state_est_wide.hpp) ask the device to do, recorded
on the CPU: tests/cpp/wide_trace.cpp runs named scenarios against the recording C ABI -- the unchanged tests/cpp/abi_recorder.cpp plus
tests/cpp/abi_recorder_wide.cpp, which defines pb_update_indexed_wide alone -- and each scenario's output must equal
tests/golden/wide_trace/<scenario>.txt byte for byte, for the plain build and for one with -fsanitize=address,undefined (the history owns,
replays and deletes the update objects)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pronto_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wide_trace")
SCENARIOS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(build):
    exe = os.path.join(ROOT, "tests", "build", "wide_trace_" + build)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    header = os.path.join(CSRC, "mav_state_est_wide.hpp")
    srcs = [os.path.join(ROOT, "tests", "cpp", f) for f in ("wide_trace.cpp", "abi_recorder.cpp", "abi_recorder_wide.cpp")]
    deps = srcs + [header, os.path.join(CSRC, "mav_state_est_batch.hpp"), os.path.join(CSRC, "mav_state_est.hpp"),
                   os.path.join(ROOT, "tests", "cpp", "abi_recorder.h"), os.path.join(ROOT, "include", "pronto_batch.h")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", '-DSHIM_HEADER="%s"' % header] + BUILDS[build]
                          + ["-o", exe] + srcs)
    return exe


def test_every_scenario_has_a_golden_trace():
    listed = subprocess.run([build_exe("plain"), "--list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(listed) == SCENARIOS and len(SCENARIOS) == 7


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_wide_trace_equals_golden(scenario, build):
    r = subprocess.run([build_exe(build), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    with open(os.path.join(GOLDEN, scenario + ".txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got, exp = r.stdout.decode(errors="replace").splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        pytest.fail("%s (%s): trace differs from line %d\n  got:    %s\n  golden: %s" % (
            scenario, build, first + 1, "\n          ".join(got[first:first + 8]), "\n          ".join(exp[first:first + 8])))
    assert r.returncode == 0
