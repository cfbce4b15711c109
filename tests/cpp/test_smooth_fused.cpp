// test_smooth_fused.cpp -- MavStateEstimator::EKFSmoothBackwardsPass with state_estimator.fuse_ins_legodo = true: the INS half of a
// fused pair has no posterior of its own, and the pass re-derives it by re-applying the pair in one fused launch with a predicted slot
// (pb_set_pred_slot).  Scenario of test_smooth_pass.cpp (host lin_rate measurements, every third step without one); every smoothed
// step against the oracle's recursion, and the smoothed posteriors of sparse checkpoints against those of a checkpoint per update,
// bit for bit.
//   argv[1]: 15 | 21 states    argv[2]: state_estimator.history_checkpoint_every (1 = every update that can have one)
//   argv[3] = "joints": instead, a joint-state log through LegOdoHandler::processMessage(joint_state_t*) (lin_rate; one robot's
//   messages for every filter, so the odometry runs inside the pair kernel), smoothed with fusion on and compared with the same run
//   with fusion off
#include <cinttypes>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../oracle/pronto_oracle.h"
#include "../../pronto_amd/csrc/mav_state_est_batch.hpp"

using namespace MavStateEst;

static uint64_t rng_state = 0x777ULL;
static double urand()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }

struct Smoothed {
  std::vector<std::vector<double>> vec, quat, cov;   // per step k: [n][B], [4][B], [n][n][B] as getHeadState gives them
};

struct Run {
  int steps = 0, calls = 0, slots = 0, status = PB_OK;
  int64_t fused = 0, reapplied = 0, pairs = 0;
  double worst = 0;
  Smoothed sm;
};

static Run run(int n, int every)
{
  rng_state = 0x777ULL;
  const int B = 20, T = 60;
  const double dt = 0.001;
  double g;
  po_get_constants(&g, nullptr);
  BotParam param;
  param.set("state_estimator.utime_history_span", "100000000");
  param.set("state_estimator.fuse_ins_legodo", "true");
  param.set("state_estimator.history_slots", (double) (every > 1 ? (2 * T) / every + every + 10 : 2 * T + 8));
  param.set("state_estimator.history_checkpoint_every", (double) every);
  RBIS x0(n, B);
  RBIM P0(n, B);
  std::vector<po_rbis> ox(B);
  std::vector<po_rbim> oP(B);
  std::vector<double> oll(B, 0.0);
  for (int b = 0; b < B; b++) {
    po_rbis_zero(&ox[b]);
    memset(&oP[b], 0, sizeof(po_rbim));
    const double sig[21] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0, .008, .008, .008, .1, .1, .1 };
    for (int i = 0; i < n; i++) { P0(i, i, b) = sig[i] * sig[i]; oP[b].m[i * 21 + i] = sig[i] * sig[i]; }
  }
  MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
  const double q4[4] = { 7.6e-5, 0.01, n == 21 ? 3e-10 : 0, n == 21 ? 1e-8 : 0 }, r_lo[3] = { 0.01, 0.01, 0.01 };
  const int vel_idx[3] = { 3, 4, 5 };
  std::vector<std::vector<po_rbis>> pred_x(T), filt_x(T);
  std::vector<std::vector<po_rbim>> pred_P(T), filt_P(T);
  for (int k = 0; k < T; k++) {
    const int64_t utime = (int64_t) (k + 1) * 1000;
    std::vector<double> imu(7 * B), lo(3 * B);
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < 3; i++) {
        imu[i * B + b] = 0.3 * sin(0.1 * k + b + i);
        imu[(3 + i) * B + b] = 0.3 * nrand() + (i == 2 ? g : 0.0);
        lo[i * B + b] = 0.1 * nrand();
      }
      imu[6 * B + b] = dt;
    }
    est.addUpdate(new RBISIMUProcessStep(std::vector<double>(imu), q4[0], q4[1], q4[2], q4[3], utime), true);
    const bool meas = (k % 3 != 2);
    if (meas)
      est.addUpdate(new RBISIndexedMeasurement(RBIS::velocityInds(), std::vector<double>(lo), std::vector<double>(r_lo, r_lo + 3),
                                               PB_R_DIAG_BROADCAST, std::vector<uint8_t>(), RBISUpdateInterface::legodo, utime), true);
    pred_x[k].resize(B); filt_x[k].resize(B); pred_P[k].resize(B); filt_P[k].resize(B);
    for (int b = 0; b < B; b++) {
      double gy[3] = { imu[b], imu[B + b], imu[2 * B + b] }, ac[3] = { imu[3 * B + b], imu[4 * B + b], imu[5 * B + b] };
      po_imu_process_step(gy, ac, dt, q4[0], q4[1], q4[2], q4[3], &ox[b], &oP[b], oll[b], &ox[b], &oP[b], &oll[b]);
      pred_x[k][b] = ox[b]; pred_P[k][b] = oP[b];
      if (meas) {
        double z[3] = { lo[b], lo[B + b], lo[2 * B + b] }, R[9] = { r_lo[0], 0, 0, 0, r_lo[1], 0, 0, 0, r_lo[2] };
        po_indexed_update(3, vel_idx, z, R, &ox[b], &oP[b], oll[b], &ox[b], &oP[b], &oll[b]);
      }
      filt_x[k][b] = ox[b]; filt_P[k][b] = oP[b];
    }
  }
  std::vector<std::vector<po_rbis>> sm_x(T);
  std::vector<std::vector<po_rbim>> sm_P(T);
  sm_x[T - 1] = filt_x[T - 1]; sm_P[T - 1] = filt_P[T - 1];
  for (int k = T - 2; k >= 0; k--) {
    sm_x[k] = filt_x[k]; sm_P[k] = filt_P[k];
    for (int b = 0; b < B; b++)
      po_ekf_smoothing_step(&pred_x[k + 1][b], &pred_P[k + 1][b], &sm_x[k + 1][b], &sm_P[k + 1][b], dt, &sm_x[k][b], &sm_P[k][b]);
  }
  Run r;
  r.sm.vec.resize(T); r.sm.quat.resize(T); r.sm.cov.resize(T);
  r.steps = est.EKFSmoothBackwardsPass(dt, [&](int64_t utime, int slot) {
    const int k = (int) (utime / 1000) - 1;
    pb_state_restore(est.ctx, slot);
    RBIS h; RBIM c;
    est.getHeadState(h, c);
    double ev = 0, sv = 0, eP = 0, sP = 0, eq = 0;
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < n; i++) { ev = fmax(ev, fabs(h(i, b) - sm_x[k][b].vec[i])); sv = fmax(sv, fabs(sm_x[k][b].vec[i])); }
      for (int i = 0; i < 4; i++) eq = fmax(eq, fabs(h.q(i, b) - sm_x[k][b].quat[i]));
      for (int cc = 0; cc < n; cc++)
        for (int rr = 0; rr < n; rr++) { eP = fmax(eP, fabs(c(rr, cc, b) - sm_P[k][b].m[cc * 21 + rr])); sP = fmax(sP, fabs(sm_P[k][b].m[cc * 21 + rr])); }
    }
    r.worst = fmax(r.worst, fmax(ev / sv, fmax(eq, eP / sP)));
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < n; i++) r.sm.vec[k].push_back(h(i, b));
      for (int i = 0; i < 4; i++) r.sm.quat[k].push_back(h.q(i, b));
      for (int cc = 0; cc < n; cc++)
        for (int rr = 0; rr < n; rr++) r.sm.cov[k].push_back(c(rr, cc, b));
    }
    r.calls++;
  });
  r.slots = est.history_slots;
  r.status = est.last_status;
  r.fused = est.fused_pairs;
  r.reapplied = est.smoother_reapplied_updates;
  r.pairs = est.smoother_reapplied_pairs;
  return r;
}

static bool same_bits(const Smoothed &a, const Smoothed &b)
{
  if (a.vec.size() != b.vec.size()) return false;
  for (size_t k = 0; k < a.vec.size(); k++)
    if (a.vec[k].size() != b.vec[k].size() || a.quat[k].size() != b.quat[k].size() || a.cov[k].size() != b.cov[k].size() ||
        memcmp(a.vec[k].data(), b.vec[k].data(), sizeof(double) * a.vec[k].size()) != 0 ||
        memcmp(a.quat[k].data(), b.quat[k].data(), sizeof(double) * a.quat[k].size()) != 0 ||
        memcmp(a.cov[k].data(), b.cov[k].data(), sizeof(double) * a.cov[k].size()) != 0)
      return false;
  return true;
}

// a biped with 6-DoF legs (test values)
static const char *URDF = R"(<?xml version="1.0"?>
<robot name="biped">
  <link name="pelvis"/><link name="l_uglut"/><link name="l_lglut"/><link name="l_uleg"/><link name="l_lleg"/><link name="l_talus"/><link name="l_foot"/>
  <link name="r_uglut"/><link name="r_lglut"/><link name="r_uleg"/><link name="r_lleg"/><link name="r_talus"/><link name="r_foot"/>
  <joint name="l_leg_hpz" type="revolute"><origin xyz="0 0.089 0" rpy="0 0 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="l_uglut"/></joint>
  <joint name="l_leg_hpx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="l_uglut"/><child link="l_lglut"/></joint>
  <joint name="l_leg_hpy" type="revolute"><origin xyz="0.05 0.0225 -0.066"/><axis xyz="0 1 0"/><parent link="l_lglut"/><child link="l_uleg"/></joint>
  <joint name="l_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374"/><axis xyz="0 1 0"/><parent link="l_uleg"/><child link="l_lleg"/></joint>
  <joint name="l_leg_aky" type="revolute"><origin xyz="0 0 -0.422"/><axis xyz="0 1 0"/><parent link="l_lleg"/><child link="l_talus"/></joint>
  <joint name="l_leg_akx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="l_talus"/><child link="l_foot"/></joint>
  <joint name="r_leg_hpz" type="revolute"><origin xyz="0 -0.089 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="r_uglut"/></joint>
  <joint name="r_leg_hpx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="r_uglut"/><child link="r_lglut"/></joint>
  <joint name="r_leg_hpy" type="revolute"><origin xyz="0.05 -0.0225 -0.066"/><axis xyz="0 1 0"/><parent link="r_lglut"/><child link="r_uleg"/></joint>
  <joint name="r_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374"/><axis xyz="0 1 0"/><parent link="r_uleg"/><child link="r_lleg"/></joint>
  <joint name="r_leg_aky" type="revolute"><origin xyz="0 0 -0.422"/><axis xyz="0 1 0"/><parent link="r_lleg"/><child link="r_talus"/></joint>
  <joint name="r_leg_akx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="r_talus"/><child link="r_foot"/></joint>
</robot>)";

struct JointRun {
  int steps = -2, status = PB_OK;
  int64_t fused = 0, leg_pairs = 0, pairs = 0;
  std::map<int64_t, std::vector<double>> sm;   // utime of INS_k -> smoothed vec | quat | cov of every filter
};

static JointRun run_joints(int n, bool fuse)
{
  rng_state = 0x4a4f494e54ULL;
  const int B = 20, T = 60, NJ = 12;
  double g;
  po_get_constants(&g, nullptr);
  BotParam param;
  param.set("state_estimator.utime_history_span", "100000000");
  param.set("state_estimator.history_slots", (double) (4 * T + 8));
  param.set("state_estimator.history_checkpoint_every", "1");
  param.set("state_estimator.fuse_ins_legodo", fuse ? "true" : "false");
  param.set("state_estimator.ins.channel", "IMU");
  param.set("state_estimator.ins.q_gyro", 0.5);
  param.set("state_estimator.ins.q_accel", 0.1);
  param.set("state_estimator.ins.timestep_dt", 0.002);
  param.set("state_estimator.ins.atlas_filter", "false");
  param.set("state_estimator.ins.q_gyro_bias", n == 21 ? 0.001 : 0.0);
  param.set("state_estimator.ins.q_accel_bias", n == 21 ? 0.0001 : 0.0);
  param.set("state_estimator.ins.accel_bias_update_online", n == 21 ? "true" : "false");
  param.set("state_estimator.ins.gyro_bias_update_online", n == 21 ? "true" : "false");
  param.applyOverrides("state_estimator.legodo.mode=lin_rate|state_estimator.legodo.r_xyz=2.0|state_estimator.legodo.r_vxyz=5|"
                       "state_estimator.legodo.r_vang=3|state_estimator.legodo.r_vxyz_uncertain=10|state_estimator.legodo.r_vang_uncertain=9|"
                       "state_estimator.legodo.schmitt_low_threshold=475|state_estimator.legodo.schmitt_high_threshold=525|"
                       "state_estimator.legodo.schmitt_low_delay=7000|state_estimator.legodo.schmitt_high_delay=7000|"
                       "state_estimator.legodo.filter_contact_events=true|state_estimator.legodo.zero_initial_velocity=3|"
                       "state_estimator.legodo.initialization_mode=zero|state_estimator.legodo.left_standing_link=l_foot|"
                       "state_estimator.legodo.right_standing_link=r_foot|state_estimator.legodo.filter_joint_positions=none|"
                       "state_estimator.legodo.total_force=900|state_estimator.legodo.standing_schmitt_level=0.65|"
                       "state_estimator.legodo.torque_adjustment=false|state_estimator.legodo.init_contact_mode=walking|"
                       "state_estimator.legodo.use_controller_input=false");
  for (const char *s : { "ins", "legodo" }) {
    param.set(std::string("state_estimator.") + s + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + s + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + s + ".utime_offset", "0");
  }
  const std::vector<std::string> names = { "l_leg_hpz", "l_leg_hpx", "l_leg_hpy", "l_leg_kny", "l_leg_aky", "l_leg_akx",
                                           "r_leg_hpz", "r_leg_hpx", "r_leg_hpy", "r_leg_kny", "r_leg_aky", "r_leg_akx" };
  ModelClient model;
  JointRun r;
  if (!model.fromURDFString(URDF, "l_foot", "r_foot")) return r;
  RBIS x0(n, B);
  RBIM P0(n, B);
  for (int b = 0; b < B; b++) {
    const double sig[21] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0, .008, .008, .008, .1, .1, .1 };
    for (int i = 0; i < n; i++) P0(i, i, b) = sig[i] * sig[i];
    x0.q(0, b) = cos(0.05 * b);
    x0.q(3, b) = sin(0.05 * b);
  }
  BotTrans ins_to_body;
  InsHandler ins_handler(&param, &ins_to_body);
  FrontEnd front_end(&param);
  auto on_ins = front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler);
  MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
  front_end.setStateEstimator(&est);
  {
    LegOdoHandler legodo_handler(&param, &model);
    auto on_joints = front_end.addSensor("legodo", &LegOdoHandler::processMessage, &legodo_handler);
    std::vector<float> jp(NJ), je(NJ, 0.f), jv(NJ, 0.f);
    double fz[2];
    for (int k = 0; k < T; k++) {
      const int64_t utime = 1000000 + (int64_t) (k + 1) * 2000;
      const double t = (k + 1) * 0.002;
      const double v[6] = { 0.2 * sin(0.05 * k), 0.05, -0.1 * cos(0.03 * k), 0.3 * nrand(), 0.3 * nrand(), g + 0.3 * nrand() };
      msgs::ins_t im{ utime, BatchArray(v, PB_HOST_BROADCAST), BatchArray(v + 3, PB_HOST_BROADCAST) };
      on_ins(&im);
      const double sw = sin(2 * M_PI * t / 0.3);
      for (int side = 0; side < 2; side++) {
        const double sgn = side ? -1.0 : 1.0, lift = fmax(0.0, -sgn * sw);
        jp[6 * side + 0] = (float) (0.05 * sgn * sw);
        jp[6 * side + 1] = (float) (0.03 * sgn);
        jp[6 * side + 2] = (float) (-0.35 - sgn * 0.2 * sw - 0.2 * lift);
        jp[6 * side + 3] = (float) (0.7 + 0.5 * lift);
        jp[6 * side + 4] = (float) (-0.35 + sgn * 0.1 * sw - 0.3 * lift);
        jp[6 * side + 5] = (float) (-0.03 * sgn);
      }
      fz[0] = 900 * (sw > -0.2 ? 1.0 : 0.1) + 5 * nrand();
      fz[1] = 900 * (sw < 0.2 ? 1.0 : 0.1) + 5 * nrand();
      msgs::six_axis_force_torque_array_t ft{ utime, BatchArray(fz, PB_HOST_BROADCAST) };
      legodo_handler.forceTorqueHandler(&ft, B);
      msgs::joint_state_t js;
      js.utime = utime;
      js.joint_name = names;
      js.joint_position = jp.data();
      js.joint_effort = je.data();
      js.joint_velocity = jv.data();
      js.mem = PB_HOST_BROADCAST;
      on_joints(&js);
    }
    est.flushPending();
    r.steps = est.EKFSmoothBackwardsPass(0.002, [&](int64_t utime, int slot) {
      pb_state_restore(est.ctx, slot);
      RBIS h; RBIM c;
      est.getHeadState(h, c);
      std::vector<double> &o = r.sm[utime];
      for (int b = 0; b < B; b++) {
        for (int i = 0; i < n; i++) o.push_back(h(i, b));
        for (int i = 0; i < 4; i++) o.push_back(h.q(i, b));
        for (int cc = 0; cc < n; cc++)
          for (int rr = 0; rr < n; rr++) o.push_back(c(rr, cc, b));
      }
    });
  }
  r.status = est.last_status;
  r.fused = est.fused_pairs;
  r.leg_pairs = est.leg_kernel_pairs;
  r.pairs = est.smoother_reapplied_pairs;
  return r;
}

static int main_joints(int n)
{
  const JointRun f = run_joints(n, true), u = run_joints(n, false);
  double worst = 0.0;
  bool same_steps = f.sm.size() == u.sm.size() && !f.sm.empty();
  for (const auto &kv : f.sm) {
    auto it = u.sm.find(kv.first);
    if (it == u.sm.end() || it->second.size() != kv.second.size()) { same_steps = false; break; }
    double e = 0.0, sc = 0.0;
    for (size_t i = 0; i < kv.second.size(); i++) { e = fmax(e, fabs(kv.second[i] - it->second[i])); sc = fmax(sc, fabs(it->second[i])); }
    worst = fmax(worst, e / sc);
  }
  printf("n=%d, joint states through LegOdoHandler: fused %d smoothing steps (%lld fused pairs, %lld in the pair kernel, %lld pairs re-applied), "
         "unfused %d steps; worst rel difference of the smoothed posteriors %.2e\n",
         n, f.steps, (long long) f.fused, (long long) f.leg_pairs, (long long) f.pairs, u.steps, worst);
  const bool ok = same_steps && f.steps > 0 && f.steps == u.steps && worst < 1e-9 && f.status == PB_OK && u.status == PB_OK && f.leg_pairs > 0 &&
                  f.pairs > 0 && u.fused == 0;
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}

int main(int argc, char **argv)
{
  const int n = (argc > 1) ? atoi(argv[1]) : 15;
  const int every = (argc > 2) ? atoi(argv[2]) : 1;
  if (argc > 3 && std::string(argv[3]) == "joints") return main_joints(n);
  const int T = 60;
  const Run r = run(n, every);
  printf("n=%d, fuse_ins_legodo, a checkpoint every %d update(s), %d slots: %d smoothing steps (%d callbacks), %lld fused pairs, "
         "%lld updates re-applied (%lld fused pairs), worst rel err vs oracle %.2e\n",
         n, every, r.slots, r.steps, r.calls, (long long) r.fused, (long long) r.reapplied, (long long) r.pairs, r.worst);
  bool ok = r.steps == T - 1 && r.calls == T - 1 && r.worst < 1e-9 && r.status == PB_OK && r.fused > 0 && r.pairs > 0;
  if (every > 1) {
    const Run r1 = run(n, 1);
    const bool same = same_bits(r.sm, r1.sm);
    printf("smoothed posteriors %s those of a checkpoint per update\n", same ? "bit-identical to" : "DIFFER from");
    ok = ok && same && r1.steps == T - 1;
  }
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
