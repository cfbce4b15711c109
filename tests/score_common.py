"""Shared by the scorer's tests: the scripted scenario, the g++ build of the per-lane functions (tests/score_host.cpp) and the
comparison of a score state ([PB_SCORE_ROWS, B] doubles + [PB_SCORE_COUNTS, B] int64) with the numpy restatement (score_ref.py).

Bounds: discrete outcomes identical; lengths in metres and angles in degrees to 1e-12 absolute -- the project's bound
for the same arithmetic in another contraction order, coordinates within +-10 m --; percent_ddt and its sums to 1e-9 relative over
windows with dist >= 0.1 m (that absolute bound divided by dist, as a percentage).  The accumulated sums are compared as the means
and root mean squares they stand for: if every term is within eps of its reference, so is the mean, and so is the rms (triangle
inequality of the 2-norm), so the same 1e-12 holds for them in metres / degrees.  The raw sums are held to the sum of their terms' bounds as well
(n x 1e-12 for sums of lengths and times, 2 n max|x| x 1e-12 for sums of squares)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ABS, TOL_PDDT = 1e-12, 1e-9


def header_enums():
    src = open(os.path.join(ROOT, "include", "pronto_batch.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(PB_SCORE_[A-Z_]+) = (\d+)", src)}


E = header_enums()
R = lambda name: E["PB_SCORE_" + name]  # noqa: E731


def build_host():
    out_dir = os.path.join(ROOT, "tests", "build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libscore_host.so")
    src = os.path.join(ROOT, "tests", "score_host.cpp")
    deps = [src, os.path.join(ROOT, "include", "pronto_batch.h")] + [os.path.join(ROOT, "pronto_amd", "csrc", h) for h in ("rbis_score.hpp", "rbis_device.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    lib = C.CDLL(so)
    lib.sh_rows.argtypes = [C.c_void_p, C.c_void_p]
    lib.sh_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.sh_message.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int64] + [C.c_void_p] * 5
    lib.sh_metric.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sh_transform_relative.argtypes = [C.c_void_p] * 3
    lib.sh_wrap_deg.argtypes, lib.sh_wrap_deg.restype = [C.c_double], C.c_double
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


class HostScore:
    """the device code's per-lane function on the host, B filters"""

    def __init__(self, lib, B, time_threshold_s=10.0, distance_threshold=0.0):
        self.lib, self.B, self.par = lib, B, (time_threshold_s, distance_threshold)
        nr, nc = C.c_int(), C.c_int()
        lib.sh_rows(C.byref(nr), C.byref(nc))
        assert (nr.value, nc.value) == (R("ROWS"), R("COUNTS"))
        self.rows, self.counts = np.zeros((nr.value, B)), np.zeros((nc.value, B), dtype=np.int64)
        lib.sh_reset(ptr(self.rows), ptr(self.counts), B)

    def message(self, utime, utimes, pose7, valid, est7, flags):
        closed = np.zeros(self.B, dtype=np.uint8)
        a = [None if x is None else np.ascontiguousarray(x, dtype=t) for x, t in ((utimes, np.int64), (pose7, np.float64), (valid, np.uint8), (est7, np.float64))]
        assert a[1].shape == (7, self.B) and a[3].shape == (7, self.B)
        self.lib.sh_message(ptr(self.rows), ptr(self.counts), self.B, *self.par, flags, int(utime), *[ptr(x) for x in a], ptr(closed))
        return closed.astype(bool)

    def metric(self, metric):
        v, has = np.zeros(self.B), np.zeros(self.B, dtype=np.uint8)
        self.lib.sh_metric(ptr(self.rows), ptr(self.counts), self.B, metric, ptr(v), ptr(has))
        return v, has.astype(bool)


def rpy_quat(roll, pitch, yaw):
    """unit quaternion (w, x, y, z) [4, ...] of a roll-pitch-yaw triple"""
    cr, sr_, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr_ * sp * sy, sr_ * cp * cy - cr * sp * sy, cr * sp * cy + sr_ * cp * sy, cr * cp * sy - sr_ * sp * cy])


STILL, YAW_CROSS = 7, 11  # the two special filters of the scenario (when B is large enough)


def scenario(B, n_msgs=120, seed=5, jitter=True, spacing_us=1_000_000):
    """n_msgs ground-truth messages for B filters, `spacing_us` apart (with +-0.2 of it of per-filter jitter in the per-filter times).
    Truth: every filter walks a circle of radius 2..8 m at 0.02..0.05 rad per message, so that its chord over the 11 messages of a
    time window is >= 0.4 m and every coordinate stays within +-10 m; its attitude is a slow roll / pitch wobble and a steady yaw rate.
    Estimate: truth plus a drift that grows by a few mm per message and a yaw error that grows by up to 0.3 deg per message.
    Filter STILL has truth that does not move (dist = 0: percent_ddt is inf, the window is left out of n_ddt); filter YAW_CROSS yaws
    by 178.2 deg per 11 messages while its estimate yaws by 182.6 deg, so its relative yaw crosses +-180 deg.  The first 5 messages
    are invalid for every third filter.  Returns a list of (utime, utimes [B], pose7 [7, B], valid [B], est7 [7, B])."""
    rng = np.random.default_rng(seed)
    rad, om, ph = rng.uniform(2, 8, B), rng.uniform(0.02, 0.05, B) * rng.choice([-1, 1], B), rng.uniform(0, 2 * np.pi, B)
    cz = rng.uniform(-1, 1, B)
    yaw_rate, yaw0 = np.radians(rng.uniform(-3, 3, B)), rng.uniform(-np.pi, np.pi, B)
    yaw_err_rate = np.radians(rng.uniform(-0.3, 0.3, B))
    drift_rate = rng.uniform(-4e-3, 4e-3, (3, B))
    if B > YAW_CROSS:
        yaw_rate[YAW_CROSS], yaw_err_rate[YAW_CROSS] = np.radians(178.2 / 11), np.radians((182.6 - 178.2) / 11)
    msgs = []
    for k in range(n_msgs):
        a = ph + om * k
        p = np.stack([rad * np.cos(a), rad * np.sin(a), cz + 0.2 * np.sin(0.1 * k + ph)])
        if B > STILL:
            p[:, STILL] = [1.5, -2.5, 0.75]
        q = rpy_quat(0.05 * np.sin(0.07 * k + ph), 0.04 * np.cos(0.05 * k + ph), yaw0 + yaw_rate * k)
        ep = p + drift_rate * k + rng.normal(0, 1e-3, (3, B))
        eq = rpy_quat(0.05 * np.sin(0.07 * k + ph) + 0.002, 0.04 * np.cos(0.05 * k + ph) - 0.001, yaw0 + (yaw_rate + yaw_err_rate) * k)
        utime = (k + 1) * spacing_us
        utimes = utime + (rng.integers(-spacing_us // 5, spacing_us // 5 + 1, B) if jitter else np.zeros(B, dtype=np.int64))
        valid = np.ones(B, dtype=np.uint8)
        if k < 5:
            valid[::3] = 0
        msgs.append((utime, utimes.astype(np.int64), np.ascontiguousarray(np.concatenate([p, q])), valid, np.ascontiguousarray(np.concatenate([ep, eq]))))
    return msgs


def check_witness(ref):
    """the scenario's own conditions, on the reference run: no compared distance within 1e-6 of the threshold (so that no discrete
    outcome hinges on rounding) and every window's distance either exactly 0 or >= 0.1 m (the range the percent_ddt bound is for)"""
    if ref.distance_threshold > 0:
        d = np.concatenate(ref.dists)
        assert d.size and np.min(np.abs(d - ref.distance_threshold)) >= 1e-6
    for w in ref.windows:
        assert np.all((w["dist"] == 0) | (w["dist"] >= 0.1))


def compare(ref, rows, counts, label=""):
    """a score state against the reference; returns the largest absolute / relative differences seen (printed by the callers)"""
    B = ref.B
    assert rows.shape == (R("ROWS"), B) and counts.shape == (R("COUNTS"), B)
    # discrete outcomes: identical
    for name, want in (("ANCHOR_UTIME", ref.last_utime), ("LAST_UTIME", ref.em_utime), ("N_WINDOWS", ref.n_windows), ("N_DDT", ref.n_ddt),
                       ("ABS_N", ref.abs_n)):
        np.testing.assert_array_equal(counts[R(name)], want, err_msg="%s %s" % (label, name))
    # the anchors are copies of inputs: identical
    a = ref.last_utime >= 0
    g, e = R("ANCHOR_GT"), R("ANCHOR_EST")
    np.testing.assert_array_equal(rows[g:g + 3, a], ref.last_p[:, a])
    np.testing.assert_array_equal(rows[g + 3:g + 7, a], ref.last_q[:, a])
    np.testing.assert_array_equal(rows[e:e + 3, a], ref.est_p[:, a])
    np.testing.assert_array_equal(rows[e + 3:e + 7, a], ref.est_q[:, a])
    worst_abs, worst_rel = 0.0, 0.0
    w = ref.n_windows > 0

    def close(got, want, what):
        nonlocal worst_abs
        if got.size:
            err = float(np.max(np.abs(got - want)))
            worst_abs = max(worst_abs, err)
            assert err <= TOL_ABS, "%s %s: %.3g" % (label, what, err)

    def close_rel(got, want, what):
        nonlocal worst_rel
        if got.size:
            err = float(np.max(np.abs(got - want) / np.abs(want)))
            worst_rel = max(worst_rel, err)
            assert err <= TOL_PDDT, "%s %s: %.3g" % (label, what, err)

    # the newest error_metrics_t
    pe, rp = R("LAST_POS_ERROR"), R("LAST_RPY_ERROR")
    close(rows[pe:pe + 3, w], ref.pos_error[:, w], "pos_error")
    close(rows[R("LAST_POS_ERROR_NORM"), w], ref.pos_error_norm[w], "pos_error_norm")
    np.testing.assert_array_equal(rows[rp:rp + 2], 0.0)
    close(rows[rp + 2, w], ref.rpy_error[2, w], "rpy_error[2]")
    close(rows[R("LAST_DISTANCE"), w], ref.distance_travelled[w], "distance_travelled")
    close(rows[R("LAST_TIME_ELAPSED"), w], ref.time_elapsed[w], "time_elapsed")
    assert np.all(rows[R("LAST_TIME_ELAPSED"), w] < 0), "time_elapsed keeps the script's (negative) sign"
    moved = w & (ref.distance_travelled >= 0.1)
    close_rel(rows[R("LAST_PERCENT_DDT"), moved], ref.percent_ddt[moved], "percent_ddt")
    still = w & (ref.distance_travelled == 0)
    assert not np.any(np.isfinite(rows[R("LAST_PERCENT_DDT"), still]))
    np.testing.assert_array_equal(rows[R("LAST_PERCENT_DDT"), still], ref.percent_ddt[still])  # the same inf / NaN
    # accumulators, as the means / root mean squares they stand for
    want = ref.derived()
    with np.errstate(divide="ignore", invalid="ignore"):
        nw, na = counts[R("N_WINDOWS")].astype(float), counts[R("ABS_N")].astype(float)
        got = dict(mean_err=rows[R("SUM_ERR")] / nw, rms_err=np.sqrt(rows[R("SUM_ERR_SQ")] / nw), max_err=rows[R("MAX_ERR")],
                   mean_distance=rows[R("SUM_DISTANCE")] / nw, mean_time=rows[R("SUM_TIME")] / nw, rms_yaw=np.sqrt(rows[R("SUM_YAW_SQ")] / nw),
                   abs_rms=np.sqrt(rows[R("ABS_SUM_SQ")] / na), abs_max=rows[R("ABS_MAX")], abs_rms_yaw=np.sqrt(rows[R("ABS_SUM_YAW_SQ")] / na))
    for k in got:
        sel = (ref.abs_n > 0) if k.startswith("abs") else w
        close(got[k][sel], want[k][sel], k)
    # ... and the raw sums themselves: n terms, each within TOL_ABS of its reference (for a square x^2, within 2 |x| TOL_ABS), can
    # differ by at most the sum of those bounds
    nwin = ref.n_windows.astype(float)
    for name, want_sum, bound in (("SUM_ERR", ref.sum_err, nwin * TOL_ABS), ("SUM_DISTANCE", ref.sum_distance, nwin * TOL_ABS),
                                  ("SUM_TIME", ref.sum_time, nwin * TOL_ABS),
                                  ("SUM_ERR_SQ", ref.sum_err_sq, 2 * nwin * ref.max_err * TOL_ABS),
                                  ("SUM_YAW_SQ", ref.sum_yaw_sq, 2 * nwin * 180.0 * TOL_ABS),
                                  ("ABS_SUM_SQ", ref.abs_sum_sq, 2 * ref.abs_n * ref.abs_max * TOL_ABS),
                                  ("ABS_SUM_YAW_SQ", ref.abs_sum_yaw_sq, 2 * ref.abs_n * 180.0 * TOL_ABS)):
        assert np.all(np.abs(rows[R(name)] - want_sum) <= bound), "%s raw %s" % (label, name)
    d = ref.n_ddt > 0
    close_rel(rows[R("SUM_PDDT"), d], ref.sum_pddt[d], "sum percent_ddt")
    close_rel(rows[R("MAX_PDDT"), d], ref.max_pddt[d], "max percent_ddt")
    np.testing.assert_array_equal(rows[R("SUM_PDDT"), ~d], 0.0)
    return worst_abs, worst_rel


def run_ref(msgs, B, time_threshold_s, distance_threshold, per_filter_times=True, use_valid=True, drift=True, absolute=True):
    """the reference over a scenario, with the per-message `closed` masks"""
    ref = sr.ScoreRef(B, time_threshold_s, distance_threshold)
    closed = [ref.message(ut if per_filter_times else u, p7[:3], p7[3:], e7[:3], e7[3:], v if use_valid else None, drift, absolute)
              for u, ut, p7, v, e7 in msgs]
    return ref, closed
