"""YawLockHandler through the C++ mirror (tests/cpp/test_yawlock.cpp): a miniature se-fusion with ins, legodo and yawlock active.

The executable checks the delayed-measurement replay itself (it equals the in-order run and leaves the yaw-lock counter alone).
For the handler-level parity with the reference chain it writes, per joint-state message, the raw status event, the gyro sample,
the joint positions, every filter's head in front of the yaw-lock update and its yaw-lock state behind it, and on sampled messages
the full prior and posterior.  Here tests/yawlock_ref.py runs on those heads -- with the standing flag derived from the raw status
events by the reference's rules, the 3-second rule of rbis_yawlock_update.cpp:146-154 included -- and the oracle's indexed
(+ orientation) update takes each sampled prior to the posterior: discrete state identical on every message and filter,
posterior within 1e-9."""
import os
import subprocess

import numpy as np
import pytest

import legs
import yawlock_ref as yr
from test_cpp_shim import build_exe
from util import rel

B, T, NJ, PERIOD, THRESHOLD = 8, 900, 16, 7, 0.4
MODES = {"yawbias": yr.YAWBIAS, "yaw": yr.YAW, "yawbias_yaw": yr.YAWBIAS_YAW, "no_such_mode": yr.YAW}


def test_shim_compiles_and_links(oracle):
    exe = build_exe(oracle, "test_yawlock")
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpronto_batch.so" in out and "not found" not in out.split("libpronto_batch.so")[1].split("\n")[0]


def standing_from_events(channel):
    """controllerStatusHandler (:125-137) / robotBehaviorHandler (:140-158) on the raw events"""
    state = dict(standing=False, last_walk=0)

    def on(kind, value, utime):
        if kind == 1:
            state["standing"] = value in (1, 8)                      # STANDING, MANIPULATING
        elif kind == 2:
            s = value in (3, 6)                                      # BEHAVIOR_STAND, BEHAVIOR_MANIPULATE
            if value == 4:                                           # BEHAVIOR_WALK
                state["last_walk"] = utime
            if utime - state["last_walk"] < 3E6:
                s = False
            state["standing"] = s
        return state["standing"]
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("n,mode,channel", [(15, "yaw", "ctrl"), (15, "no_such_mode", "ihmc"), (21, "yaw", "ihmc"), (21, "yawbias", "ctrl"),
                                            (21, "yawbias_yaw", "ctrl"), (21, "yawbias_yaw", "ihmc")])
def test_handler_against_reference_chain_and_replay(oracle, tmp_path, n, mode, channel):
    exe = build_exe(oracle, "test_yawlock")
    dump = str(tmp_path / "yawlock.bin")
    r = subprocess.run([exe, dump, mode, channel, "n%d" % n], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    if n == 15 or mode in ("yaw", "no_such_mode"):
        assert mode != "no_such_mode" or "Unrecognized" in r.stdout     # falls back to yaw like the reference
    data = np.fromfile(dump)
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    # yaw_slip_disable_period comes from the key yaw_slip_threshold_degrees (rbis_yawlock_update.cpp:19)
    ref = yr.YawLockRef(B, chain, MODES[mode], PERIOD, True, THRESHOLD, THRESHOLD, 0.05, 1.0)
    on_event = standing_from_events(channel)
    standing, at, n_full, n_standing, worst = False, 0, 0, 0, 0.0
    full_len = B * (n + 4 + n * n)
    seen = np.zeros(8, dtype=np.int64)
    for k in range(T):
        head = data[at:at + 7 + NJ]
        assert head[0] == k
        utime, full = int(head[1]), head[6] == 1.0
        if head[2] != 0:
            standing = on_event(int(head[2]), int(head[3]), int(head[4]))
        n_standing += standing
        jp = np.tile(head[7:7 + NJ].astype(np.float32)[:, None], (1, B))
        per = data[at + 7 + NJ:at + 7 + NJ + 12 * B].reshape(B, 12)
        at += 7 + NJ + 12 * B
        vec = np.zeros((21, B))
        vec[9:12] = per[:, 0:3].T
        vec[17] = per[:, 7]
        quat = np.ascontiguousarray(per[:, 3:7].T)
        z, q, mask = ref.process(standing, head[5], vec, quat, utime, jp)
        want = np.stack([ref.counter, ref.lock_init.astype(np.int64), ref.disable_until, ref.outcome | (ref.slips << 8)], axis=1)
        assert np.array_equal(per[:, 8:12].astype(np.int64), want), "message %d: yaw-lock state differs\n%s\n%s" % (k, per[:, 8:12], want)
        seen += np.bincount(ref.outcome, minlength=8)
        if full:
            blk = data[at:at + 2 * full_len].reshape(2, B, n + 4 + n * n)
            at += 2 * full_len
            v21 = np.zeros((21, B)); v21[:n] = blk[0, :, :n].T
            P21 = np.zeros((21, 21, B)); P21[:n, :n] = blk[0, :, n + 4:].reshape(B, n, n).transpose(1, 2, 0)
            ob = oracle.OracleBatch(v21, np.ascontiguousarray(blk[0, :, n:n + 4].T), P21)
            ref.apply_oracle(ob, z, q, mask)
            post_v, post_q = blk[1, :, :n].T, blk[1, :, n:n + 4].T
            post_P = blk[1, :, n + 4:].reshape(B, n, n).transpose(1, 2, 0)
            worst = max(worst, rel(post_v, ob.vec[:n]), rel(post_q, ob.quat), rel(post_P, ob.cov[:n, :n]))
            n_full += 1
    assert at == data.size
    print("n=%d %s %s: %d sampled messages, largest posterior difference %.3g; outcomes %s" % (n, mode, channel, n_full, worst, seen))
    assert worst <= 1e-9
    assert 0 < n_standing < T
    if channel == "ihmc":
        assert n_standing == T - 600    # BEHAVIOR_WALK at 0.005 s: the STAND messages up to 2.5 s fall under the 3-second rule
    if MODES[mode] != yr.YAWBIAS:
        for o in (yr.PERIOD, yr.NOT_STANDING, yr.CAPTURE, yr.CORRECTION):
            assert seen[o] > 0, "the scenario never reaches outcome %d" % o
        assert seen[yr.SLIP] > 0 and seen[yr.HOLDOFF] > 0
