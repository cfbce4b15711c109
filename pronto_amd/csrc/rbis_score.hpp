// rbis_score.hpp -- drift per distance travelled against ground truth for one filter per lane: the reference's accuracy
// evaluation, which compares POSE_BODY with POSE_GROUND_TRUTH window by window.
//
// Restatement of (paths relative to the reference tree)
//   motion_estimate/scripts/drift_per_distance.py:59-68    decide_new_measurement               -> the window test of score_message
//   motion_estimate/scripts/drift_per_distance.py:70-138   on_pose_gt                           -> score_message
//   motion_estimate/python/botpy/botpy.py:30-35            transform_relative                   -> score_transform_relative
//   motion_estimate/python/botpy/botpy.py:37-58            trans_apply_trans, trans_invert      -> score_trans_apply_trans, score_trans_invert
//   motion_estimate/python/botpy/botpy.py:60-88            quat_rotate, quat_rotate_rev, quat_mult -> score_quat_rotate (cross-product form), score_quat_rotate_rev, quat_mul (rbis_device.hpp)
//   motion_estimate/python/botpy/botpy.py:135-146          quat_to_euler (the yaw only)         -> score_yaw
// Quaternions are (w, x, y, z) and are NOT normalised anywhere, as in the script: trans_invert conjugates instead of inverting and
// quat_rotate_rev is the double product conj(q) (0, v) q, so a ground-truth quaternion of norm s scales lengths by s^2 there too.
//
// What is kept from the script as it is: the strict time comparison; `last.utime < 0` means "no anchor yet"; the yaw error is the
// plain difference of two yaws in degrees, not wrapped; percent_ddt is the IEEE quotient (dist = 0 gives inf or NaN); and
// time_elapsed = (last.utime - utime) 1e-6 is NEGATIVE (drift_per_distance.py:131 subtracts the wrong way round).
// Additions: the distance threshold the script carries commented out (:62-63), the accumulators, and the absolute error (PB_SCORE_ABS).
//
// Per-filter state: PB_SCORE_ROWS doubles + PB_SCORE_COUNTS 64-bit words (enum pb_score_row / pb_score_count, pronto_batch.h),
// struct-of-arrays, filter index fastest.  score_message touches only what the message changes: a message that closes no window
// reads the anchor position and its time and writes nothing of the drift rows.
#pragma once

#include <stdint.h>

#include "../../include/pronto_batch.h"
#include "rbis_device.hpp"

namespace pb {

struct ScorePar {
  double time_threshold_s = 10.0;     // parameterTimeElapsedThreshold (drift_per_distance.py:40)
  double distance_threshold = 0.0;    // parameterDDTThreshold (:39, 0.25 in the script, where its use is commented out); 0 = off
};

struct ScorePose {
  double t[3], q[4];
};

// botpy.quat_rotate for q = (w, u): v + 2 (w (u x v) + u x (u x v)).  For a unit quaternion this is the rotation; for any other it
// is what the script computes (the off-identity part scales with |q|^2), which is what has to be matched.
PB_HD void score_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
PB_HD void score_quat_rotate(const double (&q)[4], const double (&v)[3], double (&o)[3])
{
  const double u[3] = { q[1], q[2], q[3] };
  double uv[3], uuv[3];
  score_cross(u, v, uv);
  score_cross(u, uv, uuv);
#pragma unroll
  for (int i = 0; i < 3; i++) o[i] = v[i] + 2.0 * (q[0] * uv[i] + uuv[i]);
}

// botpy.quat_rotate_rev: the vector part of conj(q) (0, v) q, two Hamilton products (quat_mul, rbis_device.hpp) -- not divided by |q|^2
PB_HD void score_quat_rotate_rev(const double (&q)[4], const double (&v)[3], double (&o)[3])
{
  const double pure[4] = { 0.0, v[0], v[1], v[2] };
  const double conj[4] = { q[0], -q[1], -q[2], -q[3] };
  double vq[4], r[4];
  quat_mul(pure, q, vq);
  quat_mul(conj, vq, r);
  o[0] = r[1]; o[1] = r[2]; o[2] = r[3];
}

// botpy.trans_invert
PB_HD void score_trans_invert(const ScorePose &in, ScorePose &out)
{
  const double neg[3] = { -in.t[0], -in.t[1], -in.t[2] };
  score_quat_rotate_rev(in.q, neg, out.t);
  out.q[0] = in.q[0]; out.q[1] = -in.q[1]; out.q[2] = -in.q[2]; out.q[3] = -in.q[3];
}

// botpy.trans_apply_trans(src1, src): src applied to src1
PB_HD void score_trans_apply_trans(const ScorePose &src1, const ScorePose &src, ScorePose &dest)
{
  double r[3];
  score_quat_rotate(src.q, src1.t, r);
  quat_mul(src.q, src1.q, dest.q);
#pragma unroll
  for (int i = 0; i < 3; i++) dest.t[i] = r[i] + src.t[i];
}

// botpy.transform_relative(pose_a, pose_b): b as seen from a
PB_HD void score_transform_relative(const ScorePose &a, const ScorePose &b, ScorePose &ab)
{
  ScorePose ia;
  score_trans_invert(a, ia);
  score_trans_apply_trans(b, ia, ab);
}

// the yaw of botpy.quat_to_euler, radians: the heading of the body x axis, atan2 of the (1,0) and (0,0) entries of the quaternion's
// rotation matrix (again without normalising)
PB_HD double score_yaw(const double (&q)[4])
{
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  return atan2(2.0 * (x * y + w * z), 1.0 - 2.0 * (y * y + z * z));
}

// degrees into (-180, 180] (the accumulators only: what the script publishes is not wrapped)
PB_HD double score_wrap_deg(double a)
{
  return a - 360.0 * ceil((a - 180.0) / 360.0);
}

PB_HD double score_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// on_pose_gt (drift_per_distance.py:70-138) for one filter b with a valid message: ground truth (t, p, q), most_recent_est (ep, eq).
// d: [PB_SCORE_ROWS][stride] doubles, iw: [PB_SCORE_COUNTS][stride] 64-bit words.  Returns 1 when the message closed a window.
PB_HD int score_message(double *d, int64_t *iw, long stride, long b, const ScorePar &par, int flags, int64_t t, const double (&p)[3],
                        const double (&q)[4], const double (&ep)[3], const double (&eq)[4])
{
  auto D = [&](int row) -> double & { return d[(long) row * stride + b]; };
  auto I = [&](int row) -> int64_t & { return iw[(long) row * stride + b]; };
  auto anchor = [&]() {  // s.last = m; s.last_est = s.most_recent_est (:80-81, :136-137)
    I(PB_SCORE_ANCHOR_UTIME) = t;
#pragma unroll
    for (int i = 0; i < 3; i++) { D(PB_SCORE_ANCHOR_GT + i) = p[i]; D(PB_SCORE_ANCHOR_EST + i) = ep[i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) { D(PB_SCORE_ANCHOR_GT + 3 + i) = q[i]; D(PB_SCORE_ANCHOR_EST + 3 + i) = eq[i]; }
  };
  int closed = 0;
  if (flags & PB_SCORE_DRIFT) {
    const int64_t last_utime = I(PB_SCORE_ANCHOR_UTIME);
    if (last_utime < 0) {  // :79
      anchor();
    } else {
      ScorePose gt_a, gt_b, se_a, se_b;
#pragma unroll
      for (int i = 0; i < 3; i++) { gt_a.t[i] = D(PB_SCORE_ANCHOR_GT + i); gt_b.t[i] = p[i]; }
      const double dist = score_norm3(p[0] - gt_a.t[0], p[1] - gt_a.t[1], p[2] - gt_a.t[2]);  // :60, :101
      const bool by_time = (double) (t - last_utime) > par.time_threshold_s * 1e6;           // :65
      const bool by_dist = par.distance_threshold > 0.0 && dist > par.distance_threshold;      // :62
      if (by_time || by_dist) {
        closed = 1;
#pragma unroll
        for (int i = 0; i < 3; i++) { se_a.t[i] = D(PB_SCORE_ANCHOR_EST + i); se_b.t[i] = ep[i]; }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          gt_a.q[i] = D(PB_SCORE_ANCHOR_GT + 3 + i); gt_b.q[i] = q[i];
          se_a.q[i] = D(PB_SCORE_ANCHOR_EST + 3 + i); se_b.q[i] = eq[i];
        }
        ScorePose gt_ab, se_ab;
        score_transform_relative(gt_a, gt_b, gt_ab);  // :89-95
        score_transform_relative(se_a, se_b, se_ab);
        const double ex = se_ab.t[0] - gt_ab.t[0], ey = se_ab.t[1] - gt_ab.t[1], ez = se_ab.t[2] - gt_ab.t[2];  // :102
        const double drift = score_norm3(ex, ey, ez);                                                        // :103
        const double pddt = 100 * drift / dist;                                                              // :104
        const double yaw_error = score_yaw(se_ab.q) * 180.0 / M_PI - score_yaw(gt_ab.q) * 180.0 / M_PI;      // :107-109
        const double elapsed = (double) (last_utime - t) * 1e-6;                                             // :131 (negative)
        // the newest window: error_metrics_t (:124-132)
        I(PB_SCORE_LAST_UTIME) = t;
        D(PB_SCORE_LAST_POS_ERROR) = ex; D(PB_SCORE_LAST_POS_ERROR + 1) = ey; D(PB_SCORE_LAST_POS_ERROR + 2) = ez;
        D(PB_SCORE_LAST_POS_ERROR_NORM) = drift;
        D(PB_SCORE_LAST_RPY_ERROR) = 0.0; D(PB_SCORE_LAST_RPY_ERROR + 1) = 0.0; D(PB_SCORE_LAST_RPY_ERROR + 2) = yaw_error;
        D(PB_SCORE_LAST_DISTANCE) = dist;
        D(PB_SCORE_LAST_PERCENT_DDT) = pddt;
        D(PB_SCORE_LAST_TIME_ELAPSED) = elapsed;
        // accumulators
        I(PB_SCORE_N_WINDOWS) += 1;
        D(PB_SCORE_SUM_ERR) += drift;
        D(PB_SCORE_SUM_ERR_SQ) += drift * drift;
        if (drift > D(PB_SCORE_MAX_ERR)) D(PB_SCORE_MAX_ERR) = drift;
        D(PB_SCORE_SUM_DISTANCE) += dist;
        D(PB_SCORE_SUM_TIME) += fabs(elapsed);
        const double yw = score_wrap_deg(yaw_error);
        D(PB_SCORE_SUM_YAW_SQ) += yw * yw;
        if (dist > 0.0) {
          I(PB_SCORE_N_DDT) += 1;
          D(PB_SCORE_SUM_PDDT) += pddt;
          if (pddt > D(PB_SCORE_MAX_PDDT)) D(PB_SCORE_MAX_PDDT) = pddt;
        }
        anchor();
      }
    }
  }
  if (flags & PB_SCORE_ABS) {
    const double e = score_norm3(ep[0] - p[0], ep[1] - p[1], ep[2] - p[2]);
    const double yw = score_wrap_deg(score_yaw(eq) * 180.0 / M_PI - score_yaw(q) * 180.0 / M_PI);
    I(PB_SCORE_ABS_N) += 1;
    D(PB_SCORE_ABS_SUM_SQ) += e * e;
    if (e > D(PB_SCORE_ABS_MAX)) D(PB_SCORE_ABS_MAX) = e;
    D(PB_SCORE_ABS_SUM_YAW_SQ) += yw * yw;
  }
  return closed;
}

// pb_score_init's state: no anchor, no window, every accumulator 0
PB_HD void score_reset(double *d, int64_t *iw, long stride, long b)
{
  for (int r = 0; r < PB_SCORE_ROWS; r++) d[(long) r * stride + b] = 0.0;
  for (int r = 0; r < PB_SCORE_COUNTS; r++) iw[(long) r * stride + b] = 0;
  iw[(long) PB_SCORE_ANCHOR_UTIME * stride + b] = -2;  // State.__init__ (:31)
  iw[(long) PB_SCORE_LAST_UTIME * stride + b] = -2;
}

// the metric pb_score_best ranks by, from a filter's accumulators; false = the filter has no data for it
PB_HD bool score_metric(const double *d, const int64_t *iw, long stride, long b, int metric, double &v)
{
  int64_t n;
  double s;
  if (metric == PB_SCORE_MEAN_PDDT) { n = iw[(long) PB_SCORE_N_DDT * stride + b]; s = d[(long) PB_SCORE_SUM_PDDT * stride + b]; }
  else if (metric == PB_SCORE_RMS_DRIFT) { n = iw[(long) PB_SCORE_N_WINDOWS * stride + b]; s = d[(long) PB_SCORE_SUM_ERR_SQ * stride + b]; }
  else { n = iw[(long) PB_SCORE_ABS_N * stride + b]; s = d[(long) PB_SCORE_ABS_SUM_SQ * stride + b]; }
  if (n <= 0) return false;
  v = (metric == PB_SCORE_MEAN_PDDT) ? s / (double) n : sqrt(s / (double) n);
  return v == v;  // a NaN ranks nowhere: such a filter counts as without data
}

}  // namespace pb
