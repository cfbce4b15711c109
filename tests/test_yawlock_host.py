"""CPU tier of the yaw-lock handler: the per-lane functions of pronto_amd/csrc/rbis_yawlock.hpp, compiled with g++
(tests/yawlock_host.cpp), against the numpy restatement of the reference (tests/yawlock_ref.py) on one scripted scenario.

Pass condition: every discrete outcome (masks = return value and row set, outcome, lock_init, counter, disable_until, slips) is
IDENTICAL and the quaternion agrees to 1e-12 (the project's bound for "same arithmetic, other contraction order"), up to its
overall sign, which the update does not see (subtractQuats)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import legs
import yawlock_ref as yr
from oracle import leg_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, DT_US = 300, 96, 100_000
PERIOD, THRESHOLD_DEG = 3, 1.5
# NB rbis_yawlock_update.cpp:19 reads yaw_slip_disable_period from the key yaw_slip_threshold_degrees: 1.5 s here
DISABLE_S = THRESHOLD_DEG


@pytest.fixture(scope="module")
def yh():
    out_dir = os.path.join(ROOT, "tests", "build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libyawlock_host.so")
    src = os.path.join(ROOT, "tests", "yawlock_host.cpp")
    deps = [src] + [os.path.join(ROOT, "pronto_amd", "csrc", h) for h in ("rbis_yawlock.hpp", "rbis_legodo.hpp", "rbis_device.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    lib = C.CDLL(so)
    lib.yh_slerp.argtypes = [C.c_double] + [C.c_void_p] * 3
    lib.yh_chain.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.yh_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.yh_message.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 12
    lib.yh_feet.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def ptr(a):
    return a.ctypes.data


class HostYawLock:
    """the device code's state machine on the host, B robots"""

    def __init__(self, lib, chain, mode, period, slip_detect, thr, disable_s):
        self.lib, self.par = lib, (mode, period, int(slip_detect), thr, disable_s)
        nl, nr, ty, rows, org, ax = chain
        self.chain = np.zeros(lib.yh_chain_bytes(), dtype=np.uint8)
        tya, rwa = np.array(ty, dtype=np.int32), np.array(rows, dtype=np.int32)
        assert lib.yh_chain(ptr(self.chain), nl, nr, ptr(tya), ptr(rwa), ptr(np.ascontiguousarray(org)), ptr(np.ascontiguousarray(ax))) == 0
        nyd, nyi = C.c_int(), C.c_int()
        lib.yh_state_rows(C.byref(nyd), C.byref(nyi))
        self.yd, self.yi = np.zeros((nyd.value, B)), np.zeros((nyi.value, B), dtype=np.int64)
        lib.yh_reset(ptr(self.yd), ptr(self.yi), B)

    def message(self, standing, gyro_z, head, bias_z, utimes, valid, jpos):
        z, q, mask = np.zeros((2, B)), np.zeros((4, B)), np.zeros((2, B), dtype=np.uint8)
        a = [np.ascontiguousarray(x, dtype=t) for x, t in ((standing, np.uint8), (gyro_z, np.float64), (head, np.float64), (bias_z, np.float64),
                                                           (utimes, np.int64), (valid, np.uint8), (jpos, np.float32))]
        self.lib.yh_message(ptr(self.chain), B, *self.par, *[ptr(x) for x in a], ptr(self.yd), ptr(self.yi), ptr(z), ptr(q), ptr(mask))
        return z, q, mask

    disable_until = property(lambda s: s.yi[0])
    counter = property(lambda s: s.yi[1])
    slips = property(lambda s: s.yi[2])
    lock_init = property(lambda s: s.yi[3] & 1)
    outcome = property(lambda s: (s.yi[3] >> 8) & 255)


def scenario(seed=11):
    """per message: standing [B], gyro z [B], head vec [21, B] / quat [4, B], utimes [B], valid [B], joints [rows, B] float32.
    Robots b % 3 == 0 slip by 2.0 deg of left hip yaw at message 45 (above the 1.5 deg threshold), b % 3 == 1 by 1.4 deg (just
    below it), b % 3 == 2 never move a joint (their two foot-inferred orientations coincide: slerp's absD >= 1 - eps branch)."""
    from pronto_amd.synth import _quat_exp, _quat_mul
    rng = np.random.default_rng(seed)
    rows = legs.ATLAS_ROWS
    base = 0.3 * rng.normal(size=(legs.N_ROWS, B))
    for side, sgn in ((0, 1.0), (1, -1.0)):
        hpz, hpx, hpy, kny, aky, akx = rows[6 * side:6 * side + 6]
        base[hpz] = 0.05 * sgn + 0.02 * rng.normal(size=B)
        base[hpx] = 0.03 * sgn + 0.01 * rng.normal(size=B)
        base[hpy] = -0.35 + 0.05 * rng.normal(size=B)
        base[kny] = 0.7 + 0.05 * rng.normal(size=B)
        base[aky] = -0.35 + 0.05 * rng.normal(size=B)
        base[akx] = -0.03 * sgn + 0.01 * rng.normal(size=B)
    grp = np.arange(B) % 3
    sway_f = rng.uniform(0.5, 1.5, B)
    q0 = _quat_exp(0.4 * rng.normal(size=(3, B)))
    p0 = rng.normal(size=(3, B))
    drift = 0.002 * rng.normal(size=(3, B))
    bias = 1e-3 * rng.normal(size=B)
    out = []
    for k in range(T):
        t = k * DT_US * 1e-6
        standing = np.full(B, not (k < 6 or 24 <= k < 30), dtype=np.uint8)
        jp = base.copy()
        moving = grp != 2
        for side in (0, 1):
            hpy, kny = rows[6 * side + 2], rows[6 * side + 3]
            jp[hpy] += np.where(moving, 0.02 * np.sin(sway_f * t), 0.0)
            jp[kny] += np.where(moving, -0.02 * np.sin(sway_f * t), 0.0)
        if k >= 45:
            jp[rows[0]] += np.where(grp == 0, np.radians(2.0), np.where(grp == 1, np.radians(1.4), 0.0))
        vec = np.zeros((21, B))
        vec[9:12] = p0 + 0.01 * t
        vec[17] = bias
        quat = _quat_mul(q0, _quat_exp(drift * k))
        valid = np.ones(B, dtype=np.uint8)
        if k % 5 == 2:
            valid[np.arange(B) % 7 == 3] = 0
        utimes = 1_000_000 + k * DT_US + np.arange(B, dtype=np.int64)
        out.append((standing, 0.01 * rng.normal(size=B), vec, quat, utimes, valid, jp.astype(np.float32)))
    return out


def quat_err(a, b):
    """largest component difference between two sets of quaternions [4, B], up to each one's overall sign"""
    return float(np.max(np.minimum(np.abs(a - b).max(axis=0), np.abs(a + b).max(axis=0))))


@pytest.mark.parametrize("mode", [yr.YAW, yr.YAWBIAS_YAW, yr.YAWBIAS])
def test_scenario_against_reference_restatement(yh, mode):
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    msgs = scenario()
    # ---- the reference alone: the conditions on the scenario ----
    ref = yr.YawLockRef(B, chain, mode, PERIOD, True, THRESHOLD_DEG, DISABLE_S)
    expect, seen, near_one, min_margin = [], np.zeros(8, dtype=np.int64), False, np.inf
    below = above = 0
    for standing, gyro, vec, quat, utimes, valid, jp in msgs:
        z, q, mask = ref.process(standing, gyro, vec, quat, utimes, jp, valid)
        expect.append((z, q, mask, ref.outcome.copy(), ref.counter.copy(), ref.lock_init.copy(), ref.disable_until.copy(), ref.slips.copy()))
        seen += np.bincount(ref.outcome[valid != 0], minlength=8)
        m = ref.last_slip_margin_deg
        min_margin = min(min_margin, m.min())
        near_one |= bool(ref.slerp_branches[0].any())
        if mode != yr.YAWBIAS:
            # a slip just below the threshold: the robots of group 1 keep correcting after message 45
            below += int(np.sum((ref.outcome == yr.CORRECTION) & (m < 0.2)))
            above += int(np.sum(ref.outcome == yr.SLIP))
    if mode == yr.YAWBIAS:
        assert seen[yr.NOT_CALLED] > 0 and not ref.counter.any()   # getCorrection is never called: the counter does not advance
    else:
        assert min_margin > 1e-6, "a slip decision of the scenario hangs on rounding: %g deg" % min_margin
        for o in (yr.PERIOD, yr.NOT_STANDING, yr.HOLDOFF, yr.CAPTURE, yr.SLIP, yr.CORRECTION):
            assert seen[o] > 0, "the scenario never reaches outcome %d" % o
        assert above >= B // 3 and below > 0
        assert near_one, "no case reaches slerp's absD >= 1 - eps branch"
        # the hold-off runs out: a robot that slipped captures and corrects again
        slipped = np.flatnonzero(ref.slips > 0)
        assert slipped.size and np.all(ref.lock_init[slipped]) and np.all(expect[-1][6][slipped] < msgs[-1][4][slipped])
        assert np.all(ref.counter[np.arange(B) % 7 == 3] < T) and np.all(ref.counter[np.arange(B) % 7 == 0] == T)
    # ---- the device code's functions on the host ----
    dev = HostYawLock(yh, chain, mode, PERIOD, True, THRESHOLD_DEG, DISABLE_S)
    worst = 0.0
    for k, (standing, gyro, vec, quat, utimes, valid, jp) in enumerate(msgs):
        z, q, mask = dev.message(standing, gyro, np.vstack([vec[9:12], quat]), vec[17], utimes, valid, jp)
        ez, eq, emask, eout, ecnt, elock, edis, eslips = expect[k]
        assert np.array_equal(mask, emask), "message %d: masks differ" % k
        assert np.array_equal(dev.outcome, eout), "message %d: outcomes differ" % k
        assert np.array_equal(dev.counter, ecnt) and np.array_equal(dev.lock_init, elock.astype(np.int64)), "message %d" % k
        assert np.array_equal(dev.disable_until, edis) and np.array_equal(dev.slips, eslips), "message %d" % k
        assert np.array_equal(z, ez), "message %d: bias measurement differs" % k
        worst = max(worst, quat_err(q, eq))
    print("mode %d: largest quaternion difference %.3g" % (mode, worst))
    assert worst <= 1e-12


def test_slerp_branches_on_hand_made_pairs(yh):
    """both helpers on pairs that take each branch: d < 0 (scale1 negated), absD >= 1 - eps (linear), and the general one"""
    def unit(v):
        v = np.array(v, dtype=np.float64)
        return v / np.linalg.norm(v)
    a = unit([0.9, 0.1, -0.3, 0.2])
    pairs = [(a, unit([0.8, 0.2, -0.2, 0.4]), (False, False)),
             (a, -unit([0.8, 0.2, -0.2, 0.4]), (False, True)),
             (a, a.copy(), (True, False)),
             (a, -a, (True, True)),
             (unit([1, 0, 0, 0]), unit([0, 0, 0, 1]), (False, False))]
    for qa, qb, want in pairs:
        for t in (0.5, 0.25):
            r, branches = yr.slerp(t, qa, qb)
            assert tuple(bool(x) for x in branches) == want
            out = np.zeros(4)
            yh.yh_slerp(t, ptr(qa), ptr(qb), ptr(out))
            assert np.max(np.abs(out - r)) <= 1e-15
    # the d < 0 pair gives the same rotation as its positive twin
    r1, _ = yr.slerp(0.5, pairs[0][0], pairs[0][1])
    r2, _ = yr.slerp(0.5, pairs[1][0], pairs[1][1])
    assert min(np.max(np.abs(r1 - r2)), np.max(np.abs(r1 + r2))) <= 1e-15


def test_kinematics_of_the_restatement_and_of_the_device_code(yh):
    """tests/yawlock_ref.fk_batch is oracle/leg_numpy.fk for many robots; the device code's standing links agree with both"""
    rng = np.random.default_rng(3)
    for left, right, rows in ((legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS), (legs.ODD_LEFT, legs.ODD_RIGHT, legs.ODD_ROWS)):
        chain = legs.chain_arrays(left, right, rows)
        nl, nr, ty, rw, org, ax = chain
        n = 8
        jp = (0.5 * rng.normal(size=(legs.N_ROWS, n))).astype(np.float32)
        bl, br = yr.feet_batch(chain, jp)
        chain_bytes = np.zeros(yh.yh_chain_bytes(), dtype=np.uint8)
        assert yh.yh_chain(ptr(chain_bytes), nl, nr, ptr(np.array(ty, dtype=np.int32)), ptr(np.array(rw, dtype=np.int32)),
                           ptr(np.ascontiguousarray(org)), ptr(np.ascontiguousarray(ax))) == 0
        for b in range(n):
            for side, (lo, cnt, Tb) in enumerate(((0, nl, bl), (nl, nr, br))):
                ang = [float(jp[rw[lo + j], b]) if ty[lo + j] != 0 else 0.0 for j in range(cnt)]
                want = leg_numpy.fk(ty[lo:lo + cnt], org[lo:lo + cnt], ax[lo:lo + cnt], ang)
                assert np.max(np.abs(Tb[b] - want)) <= 1e-13
            feet = np.zeros(14)
            yh.yh_feet(ptr(chain_bytes), n, ptr(jp), b, ptr(feet))
            for side, Tb in enumerate((bl, br)):
                assert np.max(np.abs(feet[7 * side:7 * side + 3] - Tb[b, :3, 3])) <= 1e-13
                q = yr.matrix_to_quat(Tb[b:b + 1, :3, :3])
                assert quat_err(feet[7 * side + 3:7 * side + 7, None], q) <= 1e-13
