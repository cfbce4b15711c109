"""numpy restatement of the reference's accuracy evaluation for B estimators at once (test infrastructure only).

Written from motion_estimate/scripts/drift_per_distance.py and the botpy.py helpers it calls (transform_relative,
trans_apply_trans, trans_invert, quat_rotate, quat_rotate_rev, quat_mult, quat_to_euler); it shares no code with
pronto_amd/csrc/rbis_score.hpp and takes another route through the pose algebra (matrices here, cross products and Hamilton
products there).  Arrays are [rows, B]; quaternions are w, x, y, z and are never normalised, as in the script.

What the script does per ground-truth message m (on_pose_gt), with most_recent_est the newest POSE_BODY:
    no anchor (s.last.utime < 0):  s.last = m, s.last_est = most_recent_est
    m.utime - s.last.utime > parameterTimeElapsedThreshold * 1e6:  publish error_metrics_t, then re-anchor
The distance test it carries commented out (:62-63), the accumulators and the absolute error are this project's additions
(include/pronto_batch.h, enum pb_score_row)."""
import numpy as np


def _skew(u):
    """[3, B] -> the cross-product matrices [3, 3, B]"""
    z = np.zeros_like(u[0])
    return np.array([[z, -u[2], u[1]], [u[2], z, -u[0]], [-u[1], u[0], z]])


def _mat(q):
    """What botpy.quat_rotate applies to a vector, as a matrix [3, 3, B]: I + 2 (w K + K K) with K the cross-product matrix of the
    vector part.  The rotation matrix when |q| = 1; the script never normalises, and neither does this."""
    K = _skew(q[1:])
    eye = np.eye(3)[:, :, None]
    return eye + 2.0 * (q[0] * K + np.einsum("ijb,jkb->ikb", K, K))


def quat_mult(a, b):
    """Hamilton product as the left-multiplication matrix of a applied to b"""
    w, x, y, z = a
    L = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    return np.einsum("ijb,jb->ib", L, b)


def quat_rotate(rot, v):
    return np.einsum("ijb,jb->ib", _mat(rot), v)


def quat_rotate_rev(rot, v):
    """the vector part of conj(q) (0, v) q = ((w^2 - u.u) I + 2 u u^T - 2 w K) v -- |q|^2 times the inverse rotation"""
    w, u = rot[0], rot[1:]
    M = (w * w - np.sum(u * u, axis=0)) * np.eye(3)[:, :, None] + 2.0 * np.einsum("ib,jb->ijb", u, u) - 2.0 * w * _skew(u)
    return np.einsum("ijb,jb->ib", M, v)


def trans_invert(t, q):
    return quat_rotate_rev(q, -t), q * np.array([1.0, -1.0, -1.0, -1.0])[:, None]


def trans_apply_trans(t1, q1, t, q):
    return quat_rotate(q, t1) + t, quat_mult(q, q1)


def transform_relative(ta, qa, tb, qb):
    ti, qi = trans_invert(ta, qa)
    return trans_apply_trans(tb, qb, ti, qi)


def yaw_deg(q):
    """quat_to_euler's yaw: the heading of the first column of _mat(q)"""
    M = _mat(q)
    return np.degrees(np.arctan2(M[1, 0], M[0, 0]))


def wrap_deg(a):
    """into (-180, 180]"""
    return 180.0 - np.mod(180.0 - a, 360.0)


class ScoreRef:
    """B copies of the script's State plus the accumulators; message() is on_pose_gt for all of them"""

    def __init__(self, B, time_threshold_s=10.0, distance_threshold=0.0):
        self.B, self.time_threshold_s, self.distance_threshold = B, time_threshold_s, distance_threshold
        self.last_utime = np.full(B, -2, dtype=np.int64)
        self.last_p, self.last_q = np.zeros((3, B)), np.zeros((4, B))
        self.est_p, self.est_q = np.zeros((3, B)), np.zeros((4, B))
        # newest error_metrics_t
        self.em_utime = np.full(B, -2, dtype=np.int64)
        self.pos_error, self.pos_error_norm, self.rpy_error = np.zeros((3, B)), np.zeros(B), np.zeros((3, B))
        self.distance_travelled, self.percent_ddt, self.time_elapsed = np.zeros(B), np.zeros(B), np.zeros(B)
        # accumulators
        self.n_windows, self.n_ddt, self.abs_n = (np.zeros(B, dtype=np.int64) for _ in range(3))
        self.sum_err, self.sum_err_sq, self.max_err, self.sum_distance, self.sum_time, self.sum_yaw_sq = (np.zeros(B) for _ in range(6))
        self.sum_pddt, self.max_pddt, self.abs_sum_sq, self.abs_max, self.abs_sum_yaw_sq = (np.zeros(B) for _ in range(5))
        # witness of the threshold test: every distance compared with distance_threshold, and every closed window's figures
        self.dists, self.windows = [], []

    def message(self, utime, p, q, est_p, est_q, valid=None, drift=True, absolute=False):
        B = self.B
        t = np.broadcast_to(np.asarray(utime, dtype=np.int64), (B,))
        p, q = np.broadcast_to(p.reshape(3, -1), (3, B)), np.broadcast_to(q.reshape(4, -1), (4, B))
        on = np.ones(B, dtype=bool) if valid is None else np.asarray(valid) != 0
        closed = np.zeros(B, dtype=bool)
        if drift:
            first = on & (self.last_utime < 0)
            rest = on & ~first
            dist = np.linalg.norm(p - self.last_p, axis=0)
            close = rest & ((t - self.last_utime).astype(np.float64) > self.time_threshold_s * 1e6)
            if self.distance_threshold > 0:
                self.dists.append(dist[rest])
                close |= rest & (dist > self.distance_threshold)
            if close.any():
                c = close
                gt_t, gt_q = transform_relative(self.last_p[:, c], self.last_q[:, c], p[:, c], q[:, c])
                se_t, se_q = transform_relative(self.est_p[:, c], self.est_q[:, c], est_p[:, c], est_q[:, c])
                drift_xyz = se_t - gt_t
                d = np.linalg.norm(drift_xyz, axis=0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    pddt = 100 * d / dist[c]
                yaw_error = yaw_deg(se_q) - yaw_deg(gt_q)
                elapsed = (self.last_utime[c] - t[c]) * 1e-6
                self.em_utime[c] = t[c]
                self.pos_error[:, c], self.pos_error_norm[c] = drift_xyz, d
                self.rpy_error[2, c] = yaw_error
                self.distance_travelled[c], self.percent_ddt[c], self.time_elapsed[c] = dist[c], pddt, elapsed
                self.n_windows[c] += 1
                self.sum_err[c] += d
                self.sum_err_sq[c] += d * d
                self.max_err[c] = np.maximum(self.max_err[c], d)
                self.sum_distance[c] += dist[c]
                self.sum_time[c] += np.abs(elapsed)
                self.sum_yaw_sq[c] += wrap_deg(yaw_error) ** 2
                moved = dist[c] > 0
                idx = np.flatnonzero(c)[moved]
                self.n_ddt[idx] += 1
                self.sum_pddt[idx] += pddt[moved]
                self.max_pddt[idx] = np.maximum(self.max_pddt[idx], pddt[moved])
                self.windows.append(dict(filters=np.flatnonzero(c), dist=dist[c].copy(), pddt=pddt.copy()))
            re = first | close
            self.last_utime[re] = t[re]
            self.last_p[:, re], self.last_q[:, re] = p[:, re], q[:, re]
            self.est_p[:, re], self.est_q[:, re] = est_p[:, re], est_q[:, re]
            closed = close
        if absolute:
            e = np.linalg.norm(est_p - p, axis=0)
            yw = wrap_deg(yaw_deg(est_q) - yaw_deg(q))
            self.abs_n[on] += 1
            self.abs_sum_sq[on] += (e * e)[on]
            self.abs_max[on] = np.maximum(self.abs_max[on], e[on])
            self.abs_sum_yaw_sq[on] += (yw * yw)[on]
        return closed

    # the derived figures the tests compare: lengths in metres and angles in degrees
    def derived(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            nw, na = self.n_windows.astype(float), self.abs_n.astype(float)
            return dict(mean_err=self.sum_err / nw, rms_err=np.sqrt(self.sum_err_sq / nw), max_err=self.max_err,
                        mean_distance=self.sum_distance / nw, mean_time=self.sum_time / nw, rms_yaw=np.sqrt(self.sum_yaw_sq / nw),
                        abs_rms=np.sqrt(self.abs_sum_sq / na), abs_max=self.abs_max, abs_rms_yaw=np.sqrt(self.abs_sum_yaw_sq / na))
