// rbis_legodo_kernels.hpp -- the stand-alone leg-odometry kernels on top of rbis_legodo.hpp: k_legodo (the odometry of one message, with
// its measurement) and k_odo_legpar (the same with per-filter noises and contact thresholds), k_leg_fk, k_legodo_reset and k_legodo_get.  Launched from pronto_batch.hip only, and included by it only: the last
// three are plain (non-template) kernels, emitted by every object that sees them.
#pragma once

#include "rbis_legodo.hpp"
#include "rbis_legpar.hpp"

namespace pb {

// One robot per lane: the odometry on its state, with the filter's own head orientation as world_to_body_ (setPoseBody,
// rbis_legodo_update.cpp:214-229), then -- optionally -- the lin_rate measurement of it.
// AHEAD: the odometry is slaved to the orientation the filter WILL have after the IMU step in `imu` / imu_bc
// (rbis_update_interface.cpp:30-52 applied to the head), computed here from the head state with the step kernels' own
// ins_update_state -- the covariance is not touched.  That lets the estimator run the IMU step and the leg-odometry update
// it produces as ONE fused kernel afterwards instead of predict, odometry, update.
// (launch bounds: without them the compiler budgets for 1024-thread blocks, 128 registers, and spills)
struct LegAhead {
  int on = 0, bcast = 0;
  const double *imu = nullptr;  // [7][B]
  double v[7] = { 0, 0, 0, 0, 0, 0, 0 };
};
// SPLIT (per-filter joint blocks, 128-thread workgroups): a second wave runs the RIGHT leg's forward kinematics for the same 64
// robots and hands the foot pose over through LDS -- half of the kinematics leaves the one wave's dependent chain.
// The body, shared by the kernel's two forms: SRC says where the noises and contact thresholds come from (rbis_legpar.hpp) -- the
// kernel arguments (k_legodo) or a per-filter block (k_odo_legpar).
template <int NS, bool SPLIT, class SRC>
static __device__ __forceinline__ void legodo_one(const double *__restrict__ st, double *__restrict__ legd, int64_t *__restrict__ legi,
                                                  long stride, int B, int64_t utime, const LegPar &par, const LegIn &in,
                                                  const LegChain *__restrict__ chain, const LegAhead &ah, int zero_delta, const LegMeasPar &mp,
                                                  double *__restrict__ delta_out, double *__restrict__ status_out,
                                                  double *__restrict__ lo_out, uint8_t *__restrict__ mask_out,
                                                  double *__restrict__ pos_out, uint8_t *__restrict__ pos_ok_out, const Consts &k,
                                                  const SRC &src)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  __shared__ double foot_r[SPLIT ? 7 : 1][64];
  const long b_raw = (long) blockIdx.x * 64 + (threadIdx.x & 63u);
  const bool live = b_raw < B;
  if (!SPLIT && !live) return;
  const long b = live ? b_raw : (long) B - 1;   // (SPLIT: no lane returns before the barrier; lanes past the batch read the last robot)
  if constexpr (SPLIT) {
    if (threadIdx.x >= 64) {   // the helper wave
      Pose T;
      leg_fk_side(in, chain, 1, b, (long) B, T);
#pragma unroll
      for (int i = 0; i < 3; i++) foot_r[i][threadIdx.x & 63u] = T.t[i];
#pragma unroll
      for (int i = 0; i < 4; i++) foot_r[3 + i][threadIdx.x & 63u] = T.q[i];
      __syncthreads();
      return;
    }
  }
  LegState s;
  leg_load(s, legd, legi, stride, b, par.world_constraint != 0);
  Pose bl, br, delta;
  float fl, fr;
  int ncl, ncr;
  double wq[4], wpos[3] = { 0.0, 0.0, 0.0 };
  for (int i = 0; i < 4; i++) wq[i] = st[S::eidx(L::OFF_QUAT + i, b)];
  if (par.world_constraint && !ah.on)
    for (int i = 0; i < 3; i++) wpos[i] = st[S::eidx(L::OFF_VEC + 9 + i, b)];
  if (ah.on) {
    double gyro[3], accel[3], dt;
    if (ah.bcast) {
      for (int i = 0; i < 3; i++) { gyro[i] = ah.v[i]; accel[i] = ah.v[3 + i]; }
      dt = ah.v[6];
    } else {
      for (int i = 0; i < 3; i++) { gyro[i] = ah.imu[(long) i * B + b]; accel[i] = ah.imu[(long) (3 + i) * B + b]; }
      dt = ah.imu[(long) 6 * B + b];
    }
    if (par.world_constraint) {  // the pose after the IMU step: the whole state propagate
      double x[NS];
#pragma unroll
      for (int i = 0; i < NS; i++) x[i] = st[S::eidx(L::OFF_VEC + i, b)];
      ins_update_state<NS>(x, wq, gyro, accel, dt, k);
      for (int i = 0; i < 3; i++) wpos[i] = x[9 + i];
    } else {                     // only the orientation after it (bit-identical to the above)
      double chi[3], bg[3] = { 0.0, 0.0, 0.0 };
      for (int i = 0; i < 3; i++) chi[i] = st[S::eidx(L::OFF_VEC + 6 + i, b)];
      if (NS == 21)
        for (int i = 0; i < 3; i++) bg[i] = st[S::eidx(L::OFF_VEC + 15 + i, b)];
      ins_update_quat<NS>(chi, bg, wq, gyro, dt, k);
    }
  }
  if constexpr (SPLIT) {
    leg_fk_side(in, chain, 0, b, (long) B, bl);
    leg_inputs_rest(in, b, (long) B, fl, fr, ncl, ncr);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; i++) br.t[i] = foot_r[i][threadIdx.x & 63u];
#pragma unroll
    for (int i = 0; i < 4; i++) br.q[i] = foot_r[3 + i][threadIdx.x & 63u];
    if (!live) return;
  } else {
    leg_inputs(in, chain, b, B, bl, br, fl, fr, ncl, ncr);
  }
  if (in.utimes != nullptr) utime = in.utimes[b];                 // this filter's own message time (independent segments)
  const bool msg_ok = in.valid == nullptr || in.valid[b] != 0;    // ... or no message at all for it
  int64_t prev = 0;
  double position[3];
  bool position_ok;
  const unsigned bo = (unsigned) b * 8u;   // the lane's byte offset in a row of the parameter block
  double status = leg_update(s, src.contact_par(par, bo), utime, bl, br, fl, fr, ncl, ncr, wq, delta, prev, wpos, position, position_ok);
  const bool zero = leg_zero_velocity(s, status) || zero_delta != 0;
  if (msg_ok) leg_store(s, legd, legi, stride, b, par.world_constraint != 0);
  else status = -1.0;
  if (zero) {  // odo_delta.setIdentity(); odo_position.setIdentity() (rbis_legodo_update.cpp:266-267)
    pose_identity(delta);
    position[0] = position[1] = position[2] = 0.0;
  }
  if (pos_out != nullptr) {
    for (int i = 0; i < 3; i++) pos_out[(long) i * B + b] = position[i];
    if (pos_ok_out != nullptr) pos_ok_out[b] = position_ok ? 1 : 0;
  }
  if (delta_out != nullptr) {
    for (int i = 0; i < 3; i++) delta_out[(long) i * B + b] = delta.t[i];
    for (int i = 0; i < 4; i++) delta_out[(long) (3 + i) * B + b] = delta.q[i];
  }
  if (status_out != nullptr) status_out[b] = status;
  if (lo_out != nullptr && mp.mode == 0) {
    LegMeas m;
    const LegMeasPar &mq = src.meas_par(mp, bo);
    leg_measurement(delta, status, utime, prev, mq.r_v2, mq.r_v2_uncertain, m);
    for (int i = 0; i < 3; i++) {
      lo_out[(long) i * B + b] = m.z[i];
      lo_out[(long) (3 + i) * B + b] = m.r;
    }
    if (mask_out != nullptr) mask_out[b] = m.valid ? 1 : 0;
  } else if (lo_out != nullptr) {  // the six-row modes: z [6][B] | R diagonal [6][B]; masks [B] (six rows) | [B] (mode 2's lin_rate fall-back)
    LegMeas6 m;
    leg_measurement6(delta, status, position, position_ok, utime, prev, src.meas_par(mp, bo), m);
    for (int i = 0; i < 6; i++) {
      lo_out[(long) i * B + b] = m.z[i];
      lo_out[(long) (6 + i) * B + b] = m.r[i];
    }
    if (mask_out != nullptr) {
      mask_out[b] = m.valid6 ? 1 : 0;
      if (mp.mode == 2) mask_out[(long) B + b] = m.valid3 ? 1 : 0;
    }
  }
}
template <int NS, bool SPLIT = false>
static __global__ __launch_bounds__(SPLIT ? 128 : 64, 2) void k_legodo(const double *__restrict__ st, double *__restrict__ legd,
                                                         int64_t *__restrict__ legi, long stride, int B, int64_t utime, LegPar par,
                                                         LegIn in, const LegChain *__restrict__ chain, LegAhead ah, int zero_delta, LegMeasPar mp,
                                                         double *__restrict__ delta_out, double *__restrict__ status_out,
                                                         double *__restrict__ lo_out, uint8_t *__restrict__ mask_out,
                                                         double *__restrict__ pos_out, uint8_t *__restrict__ pos_ok_out, Consts k)
{
  legodo_one<NS, SPLIT>(st, legd, legi, stride, B, utime, par, in, chain, ah, zero_delta, mp, delta_out, status_out, lo_out, mask_out, pos_out,
                        pos_ok_out, k, LegParArgs());
}
// ... with the noises and contact thresholds per filter (pb_legodo_set_param_block)
template <int NS, bool SPLIT = false>
static __global__ __launch_bounds__(SPLIT ? 128 : 64, 2) void k_odo_legpar(const double *__restrict__ st, double *__restrict__ legd,
                                                         int64_t *__restrict__ legi, long stride, int B, int64_t utime, LegPar par,
                                                         LegIn in, const LegChain *__restrict__ chain, LegAhead ah, int zero_delta, LegMeasPar mp,
                                                         double *__restrict__ delta_out, double *__restrict__ status_out,
                                                         double *__restrict__ lo_out, uint8_t *__restrict__ mask_out,
                                                         double *__restrict__ pos_out, uint8_t *__restrict__ pos_ok_out, Consts k,
                                                         LegParRows rows)
{
  legodo_one<NS, SPLIT>(st, legd, legi, stride, B, utime, par, in, chain, ah, zero_delta, mp, delta_out, status_out, lo_out, mask_out, pos_out,
                        pos_ok_out, k, rows);
}
// forward kinematics alone: feet_out [14][B] (diagnostics, tests)
static __global__ __launch_bounds__(64) void k_leg_fk(LegIn in, const LegChain *__restrict__ chain, int B, double *__restrict__ feet_out)
{
  const long b = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Pose bl, br;
  float fl, fr;
  int ncl, ncr;
  leg_inputs(in, chain, b, B, bl, br, fl, fr, ncl, ncr);
  for (int i = 0; i < 3; i++) { feet_out[(long) i * B + b] = bl.t[i]; feet_out[(long) (7 + i) * B + b] = br.t[i]; }
  for (int i = 0; i < 4; i++) { feet_out[(long) (3 + i) * B + b] = bl.q[i]; feet_out[(long) (10 + i) * B + b] = br.q[i]; }
}
// zero_ticks < 0: reset everything; otherwise only set the per-robot zero_initial_velocity counter
static __global__ void k_legodo_reset(double *legd, int64_t *legi, long stride, int B, int zero_ticks)
{
  const long b = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  LegState s;
  if (zero_ticks < 0) leg_reset(s);
  else {
    leg_load(s, legd, legi, stride, b, true);
    s.zero_ticks = zero_ticks > 65535 ? 65535 : zero_ticks;
  }
  leg_store(s, legd, legi, stride, b, true);
}
static __global__ void k_legodo_get(const double *legd, const int64_t *legi, long stride, long b, double *pose7, int64_t *info)
{
  LegState s;
  leg_load(s, legd, legi, stride, b);
  for (int i = 0; i < 3; i++) pose7[i] = s.body_t[i];
  for (int i = 0; i < 4; i++) pose7[3 + i] = s.body_q[i];
  info[0] = s.primary_foot; info[1] = s.leg_odo_init; info[2] = s.mode; info[3] = s.unknown_transitions;
}

}  // namespace pb
