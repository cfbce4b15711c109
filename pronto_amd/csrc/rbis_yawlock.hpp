// rbis_yawlock.hpp -- the yaw-lock handler for one filter per lane: while the robot stands, the two feet do not move in the
// world, so the pelvis orientation that follows from the pose the feet had when the robot came to stand (and the leg
// kinematics now) is a drift-free measurement of yaw, and the body-frame gyro z is a measurement of the gyro bias z.
//
// Restatement of (paths relative to the reference tree)
//   motion_estimate/src/quick_lock/yawlock.cpp:78-205             YawLock::getCorrection            -> yaw_get_correction
//   motion_estimate/src/quick_lock/yawlock.hpp                    the members that make up the state -> YawState
//   motion_estimate/src/quick_lock/rbis_yawlock_update.cpp:168-232   YawLockHandler::processMessage  -> yaw_form
//   pronto-utils/src/pronto_math/pronto_math.cpp:53-61            quat_to_euler                     -> quat_to_rpy (rbis_legodo.hpp)
//   Eigen 3.3 Quaterniond::slerp (Eigen is NOT in the tree; the published algorithm)               -> yaw_slerp
// Poses are (translation, unit quaternion) pairs as in rbis_legodo.hpp, where the reference holds Eigen::Isometry3d and
// turns rotation matrices into quaternions (yawlock.cpp:150-153,177-178): the quaternion that comes out here may have the
// other overall sign.  The update takes it through subtractQuats, which does not see that sign.
//
// Per-filter state: NYD doubles + NYI 64-bit words, struct-of-arrays, filter index fastest.  `standing` and the gyro sample
// are inputs (the status / IMU handlers set them), not state.
#pragma once

#include <stdint.h>

#include "rbis_legodo.hpp"

namespace pb {

enum { YL_YAWBIAS = 0, YL_YAW = 1, YL_YAWBIAS_YAW = 2 };  // YawLockMode (rbis_yawlock_update.hpp)
// what the last message did to a filter (pb_yawlock_get): where getCorrection returned
enum {
  YO_NO_MESSAGE = 0,    // valid == 0, or nothing received yet
  YO_PERIOD = 1,        // yawlock.cpp:82-85   not a correction tick
  YO_NOT_STANDING = 2,  // yawlock.cpp:88-92
  YO_HOLDOFF = 3,       // yawlock.cpp:94-99   disabled after a slip
  YO_CAPTURE = 4,       // yawlock.cpp:123-138 the lock was initialised
  YO_SLIP = 5,          // yawlock.cpp:152-171
  YO_CORRECTION = 6,    // yawlock.cpp:204     returned true
  YO_NOT_CALLED = 7     // mode yawbias: getCorrection is never called (rbis_yawlock_update.cpp:186)
};

struct YawPar {
  int mode = YL_YAW, period = 1, slip_detect = 0;
  double slip_threshold_deg = 0.0;
  double slip_disable_s = 0.0;  // NB the reference reads it from the key ...yaw_slip_threshold_degrees (rbis_yawlock_update.cpp:19)
  double r_bias = 0.0, r_yaw = 0.0;  // variances: (r_yaw_bias pi/180)^2, (r_yaw pi/180)^2 (rbis_yawlock_update.cpp:80,88)
};

struct YawState {
  Pose world_to_l, world_to_r;  // world_to_{l,r}_foot_original_
  double lr_q[4];               // rotation of l_foot_to_r_foot_original_ (only its yaw is ever read, yawlock.cpp:149)
  int64_t disable_until;        // utime_disable_until_
  int64_t counter;              // counter_
  int64_t slips;                // slips detected so far (the reference publishes YAW_SLIP_DETECTED instead)
  int lock_init, outcome;       // lock_init_ | YO_*
};
static constexpr int NYD = 18, NYI = 4;  // words: disable_until, counter, slips, lock_init | outcome << 8

// the constructor's state (yawlock.cpp:60-65)
PB_HD void yaw_reset(YawState &s)
{
  pose_identity(s.world_to_l);
  pose_identity(s.world_to_r);
  s.lr_q[0] = 1.0; s.lr_q[1] = s.lr_q[2] = s.lr_q[3] = 0.0;
  s.disable_until = 0;
  s.counter = 0;
  s.slips = 0;
  s.lock_init = 0;
  s.outcome = YO_NO_MESSAGE;
}

// Eigen 3.3 QuaternionBase::slerp(t, other) on a = *this, b = other (component order w, x, y, z here)
PB_HD void yaw_slerp(double t, const double (&a)[4], const double (&b)[4], double (&o)[4])
{
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[0] * b[0];
  const double ad = fabs(d);
  double s0, s1;
  if (ad >= one) {
    s0 = 1.0 - t;
    s1 = t;
  } else {
    const double th = acos(ad), sn = sin(th);
    s0 = sin((1.0 - t) * th) / sn;
    s1 = sin(t * th) / sn;
  }
  if (d < 0.0) s1 = -s1;
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = s0 * a[i] + s1 * b[i];
}

// YawLock::getCorrection (yawlock.cpp:78-205).  `feet(bl, br)` evaluates the two standing links (body_to_l_foot,
// body_to_r_foot); it is called only where the reference runs the kinematics solver, i.e. not on the period - 1 of period
// messages that leave at the counter.
template <class FEET>
PB_HD bool yaw_get_correction(YawState &s, const YawPar &p, bool standing, const Pose &world_to_body, int64_t utime, FEET &&feet,
                              double (&q_out)[4])
{
  const bool tick = (s.counter % p.period) == 0;  // yawlock.cpp:82
  s.counter++;
  if (!tick) { s.outcome = YO_PERIOD; return false; }
  if (!standing) {  // yawlock.cpp:88-92
    s.lock_init = 0;
    s.outcome = YO_NOT_STANDING;
    return false;
  }
  if (p.slip_detect && utime < s.disable_until) { s.outcome = YO_HOLDOFF; return false; }  // yawlock.cpp:94-99
  Pose bl, br, bl_inv, lr;
  feet(bl, br);
  pose_inv(bl, bl_inv);
  pose_mul(bl_inv, br, lr);  // yawlock.cpp:120
  if (!s.lock_init) {        // yawlock.cpp:123-138
    pose_mul(world_to_body, bl, s.world_to_l);
    pose_mul(world_to_body, br, s.world_to_r);
#pragma unroll
    for (int i = 0; i < 4; i++) s.lr_q[i] = lr.q[i];
    s.lock_init = 1;
    s.outcome = YO_CAPTURE;
    return false;
  }
  if (p.slip_detect) {  // yawlock.cpp:142-172: fabs of the PLAIN difference of the two yaws (not wrapped)
    double now[3], orig[3];
    quat_to_rpy(lr.q, now);
    quat_to_rpy(s.lr_q, orig);
    const double change = fabs(now[2] - orig[2]);
    if (change * 180 / M_PI > p.slip_threshold_deg) {
      s.disable_until = (int64_t) ((double) utime + p.slip_disable_s * 1E6);  // yawlock.cpp:153
      s.lock_init = 0;
      s.slips++;
      s.outcome = YO_SLIP;
      return false;
    }
  }
  // the mean of the orientations inferred by the two feet (yawlock.cpp:175-180)
  Pose br_inv, using_l, using_r;
  pose_inv(br, br_inv);
  pose_mul(s.world_to_l, bl_inv, using_l);
  pose_mul(s.world_to_r, br_inv, using_r);
  yaw_slerp(0.5, using_l.q, using_r.q, q_out);
  s.outcome = YO_CORRECTION;
  return true;
}

// YawLockHandler::processMessage (rbis_yawlock_update.cpp:168-232) for one filter.
//   head: position and quaternion of the filter's head state; bias_z: its gyro bias z (0 for 15 states, where only mode
//   yaw exists); gyro_z: the last body-frame gyro z insHandler kept.
//   z[0] = the bias measurement (the reference passes it with every row set; the chi row's residual comes from q);
//   mask[0] = apply the mode's row set with the orientation q ({chi z} / {gyro bias z, chi z}),
//   mask[1] = apply the gyro-bias row alone.  Neither = the handler returned NULL.
template <class FEET>
PB_HD void yaw_form(YawState &s, const YawPar &p, bool standing, double gyro_z, const Pose &head, double bias_z, int64_t utime,
                    FEET &&feet, double (&z)[2], double (&q)[4], bool (&mask)[2])
{
  z[0] = standing ? gyro_z : bias_z;  // rbis_yawlock_update.cpp:177-182
  z[1] = 0.0;
  q[0] = 1.0; q[1] = q[2] = q[3] = 0.0;
  bool valid = false;
  if (p.mode == YL_YAW || p.mode == YL_YAWBIAS_YAW) valid = yaw_get_correction(s, p, standing, head, utime, feet, q);  // :187-190
  else s.outcome = YO_NOT_CALLED;  // (the counter does not advance in mode yawbias)
  mask[0] = valid;
  mask[1] = (p.mode == YL_YAWBIAS) || (p.mode == YL_YAWBIAS_YAW && !valid);  // :195-199, :212-224
}

// SoA <-> struct (filter index fastest; d: [NYD][stride] doubles, iw: [NYI][stride] 64-bit words)
PB_HD void yaw_load(YawState &s, const double *d, const int64_t *iw, long stride, long b)
{
#pragma unroll
  for (int i = 0; i < 3; i++) { s.world_to_l.t[i] = d[(long) i * stride + b]; s.world_to_r.t[i] = d[(long) (7 + i) * stride + b]; }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    s.world_to_l.q[i] = d[(long) (3 + i) * stride + b];
    s.world_to_r.q[i] = d[(long) (10 + i) * stride + b];
    s.lr_q[i] = d[(long) (14 + i) * stride + b];
  }
  s.disable_until = iw[b];
  s.counter = iw[stride + b];
  s.slips = iw[2 * stride + b];
  const int64_t w = iw[3 * stride + b];
  s.lock_init = (int) (w & 1);
  s.outcome = (int) ((w >> 8) & 255);
}
// `poses`: also the captured poses (they change on a capture only)
PB_HD void yaw_store(const YawState &s, double *d, int64_t *iw, long stride, long b, bool poses = true)
{
  if (poses) {
#pragma unroll
    for (int i = 0; i < 3; i++) { d[(long) i * stride + b] = s.world_to_l.t[i]; d[(long) (7 + i) * stride + b] = s.world_to_r.t[i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      d[(long) (3 + i) * stride + b] = s.world_to_l.q[i];
      d[(long) (10 + i) * stride + b] = s.world_to_r.q[i];
      d[(long) (14 + i) * stride + b] = s.lr_q[i];
    }
  }
  iw[b] = s.disable_until;
  iw[stride + b] = s.counter;
  iw[2 * stride + b] = s.slips;
  iw[3 * stride + b] = (int64_t) (s.lock_init & 1) | ((int64_t) s.outcome << 8);
}

// one message's inputs beside the joint state (LegIn): what the status and IMU handlers keep, per filter or one for all
struct YawIn {
  const uint8_t *standing = nullptr;  // [B] (device) or NULL: standing_all
  const double *gyro_z = nullptr;     // [B] (device) or NULL: gyro_z_all
  int standing_all = 0;
  double gyro_z_all = 0.0;
};

// the two standing links of filter b from the message (a broadcast joint state arrives as the two transforms, rbis_legodo.hpp)
PB_HD void yaw_feet(const LegIn &in, const LegChain *chain, long b, long B, Pose &bl, Pose &br)
{
  if (in.kind == 0) {
#pragma unroll
    for (int i = 0; i < 3; i++) { bl.t[i] = in.v[i]; br.t[i] = in.v[7 + i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) { bl.q[i] = in.v[3 + i]; br.q[i] = in.v[10 + i]; }
  } else {
    leg_fk_side(in, chain, 0, b, B, bl);
    leg_fk_side(in, chain, 1, b, B, br);
  }
}

}  // namespace pb
