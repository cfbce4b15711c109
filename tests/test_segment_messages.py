"""What SegmentBatcher and SegmentStreamer hand to the handlers, on the CPU: tests/cpp/segment_messages.cpp writes a small set of logs,
replays them through both replayers against host stand-ins for the C ABI (make_stubs of tests/test_host_sanitizers.py) and prints every
batched message -- every member of every column, bit for bit -- and the integer counters.

Golden comparison.  Each trace must equal tests/golden/segment_messages/<name>.txt byte for byte, in a plain build and in one with
-fsanitize=address,undefined.  The goldens were recorded with segment_batcher.hpp and segment_stream.hpp as they were before the channel
decoders and the result keeper moved into segment_channels.hpp; they are the record that the move changed nothing either replayer hands
over, and they are not to be regenerated from headers they are meant to check.

Cross-check.  For each IMU channel the batcher's trace is compared with the streamer's max_slots = 96 trace of the same logs: message
order, channels, batch utimes, joint names, prev_timestamp, max_new, the valid masks, the values and per-filter utimes of valid columns,
and the counters batches and per_channel.  Left out, because the two replayers differ there by design:
  * masked columns: the batcher's blocks keep a column's last value per block and its KVH / joint utimes are 0; the streamer repeats
    the segment's last record on the channel;
  * force/torque: the batcher hands over signed doubles, the streamer (float) fabs(): compared as such (it has no mask: every column);
  * undecodable, order_violations, ragged, max_skew_us, readahead_capped: counted per replayer (KVH overflow and foreign joint lists
    are counted in different places, order is judged per message by one and per chunk by the other);
  * segment_messages: the batcher's is one higher.  It counts the message with the foreign joint list as carried and masks it at
    dispatch (into undecodable); the streamer rejects it in the decoder.  Asserted as such.
The streamer's lines have no column 4: it never writes the columns behind its last segment, and they hold what the ring buffer's last
use left there (which buffer that was depends on the timing of its two threads), so there is nothing stable to record."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_sanitizers import make_stubs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "segment_messages")
TRACES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]}
NSEG = 4   # segments in the batch of 5
_ran = {}


def run_harness(build, tmp_path_factory):
    """the traces of one build, {name: bytes}; built and run once per session"""
    if build in _ran:
        return _ran[build]
    bdir = os.path.join(ROOT, "tests", "build")
    os.makedirs(bdir, exist_ok=True)
    stubs = os.path.join(bdir, "segment_messages_stubs.cpp")
    assert make_stubs(stubs) >= 70
    exe = os.path.join(bdir, "segment_messages_" + build)
    src = os.path.join(ROOT, "tests", "cpp", "segment_messages.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Werror=return-type"] + BUILDS[build] + ["-o", exe, src, stubs])
    out = tmp_path_factory.mktemp("segment_messages_" + build)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    traces = {}
    for f in os.listdir(str(out)):
        if f.endswith(".txt"):
            with open(os.path.join(str(out), f), "rb") as fh:
                traces[f[:-4]] = fh.read()
    _ran[build] = traces
    return traces


def test_every_trace_has_a_golden(tmp_path_factory):
    assert sorted(run_harness("plain", tmp_path_factory)) == TRACES and len(TRACES) == 9


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("trace", TRACES)
def test_segment_messages_equal_golden(trace, build, tmp_path_factory):
    got = run_harness(build, tmp_path_factory)[trace]
    with open(os.path.join(GOLDEN, trace + ".txt"), "rb") as f:
        want = f.read()
    if got != want:
        g, w = got.decode(errors="replace").splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail("%s (%s): trace differs from line %d\n  got:    %s\n  golden: %s" % (trace, build, first + 1, g[first:first + 1], w[first:first + 1]))


def parse(trace):
    """-> (messages, counters): a message is (channel, utime, {extra member: text}, [per column {member: text}])"""
    msgs, counters = [], {}
    for line in trace.decode().splitlines():
        head, *cols = line.split(" ; ")
        words = head.split()
        if words[0] in ("stats", "per_channel", "final_utime") or "=" in words[0]:
            counters.update(dict(w.split("=") for w in words if "=" in w))
            if words[0] == "final_utime":
                counters["final_utime"] = words[1:]
            continue
        extra = dict(w.split("=") for w in words[2:])
        members = extra.pop("members").split(",")
        msgs.append((words[0], words[1], extra, [None if c == "-" else dict(zip(members, c.split(), strict=True)) for c in cols]))
    return msgs, counters


def as_float_abs(text):
    return struct.unpack("f", struct.pack("f", abs(float.fromhex(text))))[0]


@pytest.mark.parametrize("imu", ["ins", "kvh_filter", "kvh_newest"])
def test_batcher_and_streamer_hand_over_the_same_messages(imu, tmp_path_factory):
    traces = run_harness("plain", tmp_path_factory)
    (bm, bc), (sm, sc) = parse(traces["batcher_" + imu]), parse(traces["streamer_%s_slots96" % imu])
    assert [m[0] for m in bm] == [m[0] for m in sm]                      # message order and channels
    assert len(bm) >= 40
    compared = 0
    for k, ((ch, ut, extra, cols), (_, s_ut, s_extra, s_cols)) in enumerate(zip(bm, sm)):
        where = "message %d (%s)" % (k, ch)
        assert len(cols) == len(s_cols) == 5, where
        if ch == "FORCE_TORQUE":                                             # (the streamer's callback carries no time and no mask)
            for c, s in zip(cols[:NSEG], s_cols[:NSEG]):
                assert [as_float_abs(x) for x in c["force_z"].split(",")] == [float.fromhex(x) for x in s["force_z"].split(",")], where
            continue
        assert ut == s_ut and extra == s_extra, where                       # batch utime; joint_name, prev_timestamp, max_new
        for c, s in zip(cols[:NSEG], s_cols[:NSEG]):
            assert c["valid"] == s["valid"], where
            if ch == "VO_UPDATE" or c["valid"] == "1":                       # (update_t's mask is the estimate's status: no column is masked
                same = dict(c) == dict(s)                                    # for having no message -- but such a column is blank in both)
                assert same, "%s: %r != %r" % (where, c, s)
                compared += 1
    assert compared > 60                                                     # (some 30 messages that are not force/torque, 2 to 4 live columns)
    for key in ["batches"] + [k for k in bc if k.isupper()]:
        assert bc[key] == sc[key], key
    assert int(bc["segment_messages"]) == int(sc["segment_messages"]) + 1
