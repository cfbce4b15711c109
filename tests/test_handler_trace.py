"""What the sensor handlers (pronto_amd/csrc/mav_state_est_batch.hpp) decide, recorded on the CPU: the driver tests/cpp/handler_trace.cpp runs
named scenarios against a recording C ABI (tests/cpp/abi_recorder.cpp: no HIP, no library) and prints, for every message handed to a handler,
the update object it returned -- class, sensor, utime, index list, memory spaces, R kind, masks, checksums of the host payloads it owns,
which deferred-measurement hooks are set, or NULL -- between the pb_* calls the handler and then the estimator made for it and the handler's
own messages; for a processMessageInit the return value and checksums of the state, the quaternions and the covariance.  Each scenario's
output must equal tests/golden/handler_trace/<scenario>.txt byte for byte, and a scenario that ends in a handler's exit() must end with
that exit code.

The golden files were written once by building the driver against the headers (mav_state_est_batch.hpp, mav_state_est.hpp, lcm_schema.hpp,
pronto_wire.hpp) of the commit BEFORE the handlers' repeated code was folded into shared helpers; they are the record that the fold changed
no decision, and they are not to be regenerated from a header they are meant to check.  The same traces are required of a stand-alone build
with -fsanitize=address,undefined: the handlers copy host rows and masks into vectors the updates own and pass device blocks around by
shared pointer.

One recorded decision is a defect that the fold left as it found it: when pb_memcpy_h2d fails while host foot forces are uploaded into a
fresh ff_pool_ block (LegOdoHandler::processMessage), the block is neither attached to the message nor given back to its pool.  The trace
of legodo_joints_failing pins that (no pb_free for the block); a change that gives the block back changes that trace on purpose."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pronto_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "handler_trace")
SCENARIOS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))
# a scenario named *_exit ends in exit(1), libbot's *_or_fail behaviour, or in the reference's own exit(-1)
EXIT_CODE = {s: 1 for s in SCENARIOS if s.endswith("_exit")}
EXIT_CODE.update({s: 255 for s in ("legodo_chain_joint_missing_exit", "legodo_adjustment_joint_missing_exit", "yawlock_channel_exit", "fovis_mode_exit")})
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(build):
    exe = os.path.join(ROOT, "tests", "build", "handler_trace_" + build)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    header = os.path.join(CSRC, "mav_state_est_batch.hpp")
    srcs = [os.path.join(ROOT, "tests", "cpp", f) for f in ("handler_trace.cpp", "abi_recorder.cpp")]
    deps = srcs + [header, os.path.join(ROOT, "tests", "cpp", "abi_recorder.h"), os.path.join(ROOT, "include", "pronto_batch.h")]
    deps += [os.path.join(CSRC, h) for h in ("mav_state_est.hpp", "lcm_schema.hpp", "pronto_wire.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", '-DSHIM_HEADER="%s"' % header] + BUILDS[build]
                          + ["-o", exe] + srcs)
    return exe


def test_every_scenario_has_a_golden_trace():
    listed = subprocess.run([build_exe("plain"), "--list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(listed) == SCENARIOS and len(SCENARIOS) >= 35
    assert all(s in SCENARIOS for s in EXIT_CODE)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_handler_trace_equals_golden(scenario, build):
    r = subprocess.run([build_exe(build), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    with open(os.path.join(GOLDEN, scenario + ".txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got, exp = r.stdout.decode(errors="replace").splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        pytest.fail("%s (%s): trace differs from line %d\n  got:    %s\n  golden: %s" % (
            scenario, build, first + 1, "\n          ".join(got[first:first + 8]), "\n          ".join(exp[first:first + 8])))
    assert r.returncode == EXIT_CODE.get(scenario, 0)
