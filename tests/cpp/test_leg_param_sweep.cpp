// test_leg_param_sweep.cpp -- LegOdoHandler::setSweep: the batch's form of the reference's `-O key=value` parameter sweep
// (state-estimator/python/param_sweep.py:39-52).  ONE robot's IMU + joint-state log drives 96 filters that differ in
// state_estimator.legodo.r_vxyz and .schmitt_high_threshold alone (setSweep -> pb_legodo_set_param_block); filters 0, 47 and 95 must be
// what a batch of ONE filter computes from the same log when its .cfg carries that filter's two values: relative 1e-12 on the head
// state, covariance and log-likelihood (whether they are bit-equal is printed).
//   argv[1]: "host" = only setSweep's argument checks (no GPU) | "fuse" | "nofuse" = state_estimator.fuse_ins_legodo
//   argv[2]: "late" = posterior checkpoints on, and on every 10th tick a VO message stamped 300 us BEFORE the leg odometry that has been
//            applied already: the estimator restores the checkpoint in front of it and re-applies the kept leg-odometry block, which
//            carries each filter's own R
//   "n21" anywhere: the 21-state filter
// Exit code 0 + "PASS".
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "test_n.hpp"

using namespace MavStateEst;

static uint64_t rng_state = 0x5357454550ULL;
static double urand()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }
static double ramp(double x) { return x < 0 ? 0 : (x > 0.05 ? 1.0 : x / 0.05); }

// a biped with 6-DoF legs (test values, as tests/cpp/test_leg_joints.cpp)
static const char *URDF = R"(<?xml version="1.0"?>
<robot name="biped">
  <link name="pelvis"><inertial><mass value="17.8"/><origin xyz="0 0 0" rpy="0 0 0"/></inertial></link>
  <link name="l_uglut"/><link name="l_lglut"/><link name="l_uleg"/><link name="l_lleg"/><link name="l_talus"/><link name="l_foot"/>
  <link name="r_uglut"/><link name="r_lglut"/><link name="r_uleg"/><link name="r_lleg"/><link name="r_talus"/><link name="r_foot"/>
  <link name="utorso"/><link name="l_sole"/>
  <joint name="back_bkz" type="revolute"><origin xyz="-0.0125 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="utorso"/>
    <limit effort="124" lower="-0.6" upper="0.6" velocity="12"/></joint>
  <joint name="l_leg_hpz" type="revolute"><origin xyz="0 0.089 0" rpy="0 0 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="l_uglut"/>
    <dynamics damping="0.1" friction="0"/><limit effort="110" lower="-0.17" upper="1.1" velocity="12"/></joint>
  <joint name="l_leg_hpx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="l_uglut"/><child link="l_lglut"/></joint>
  <joint name="l_leg_hpy" type="revolute"><origin rpy="0 0 0" xyz="0.05 0.0225 -0.066"/><axis xyz="0 1 0"/><parent link="l_lglut"/><child link="l_uleg"/></joint>
  <joint name="l_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374" rpy="0 0.02 0"/><axis xyz="0 1 0"/><parent link="l_uleg"/><child link="l_lleg"/></joint>
  <joint name="l_leg_aky" type="continuous"><origin xyz="0 0 -0.422" rpy="0 0 0"/><axis xyz="0 1 0"/><parent link="l_lleg"/><child link="l_talus"/></joint>
  <joint name="l_leg_akx" type="revolute"><origin xyz="0 0 0" rpy="0 0 0"/><parent link="l_talus"/><child link="l_foot"/></joint>
  <joint name="l_sole_fixed" type="fixed"><origin xyz="0.05 0 -0.081" rpy="0 0 0"/><parent link="l_foot"/><child link="l_sole"/></joint>
  <joint name="r_leg_hpz" type="revolute"><origin xyz="0 -0.089 0" rpy="0 0 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="r_uglut"/></joint>
  <joint name="r_leg_hpx" type="revolute"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/><parent link="r_uglut"/><child link="r_lglut"/></joint>
  <joint name="r_leg_hpy" type="revolute"><origin xyz="0.05 -0.0225 -0.066" rpy="0 0 0"/><axis xyz="0 1 0"/><parent link="r_lglut"/><child link="r_uleg"/></joint>
  <joint name="r_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374" rpy="0 0.02 0"/><axis xyz="0 1 0"/><parent link="r_uleg"/><child link="r_lleg"/></joint>
  <joint name="r_leg_aky" type="revolute"><origin xyz="0 0 -0.422" rpy="0 0 0"/><axis xyz="0 1 0"/><parent link="r_lleg"/><child link="r_talus"/></joint>
  <joint name="r_leg_akx" type="revolute"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/><parent link="r_talus"/><child link="r_foot"/></joint>
  <transmission name="l_leg_kny_trans" type="pr2_mechanism_model/SimpleTransmission"><actuator name="l_leg_kny_motor"/><joint name="l_leg_kny"/>
    <mechanicalReduction>1</mechanicalReduction></transmission>
</robot>)";


enum { T = 700, NJ = 16 };
// the one robot's log, made once: every run replays the same numbers
struct Tick {
  double imu[6], fz[2], vo_t[3], vo_q[4];
  float jp[NJ], je[NJ];
};
struct Head {
  std::vector<double> v;   // vec | quat | cov | log-likelihood of one filter
};
struct Run {
  std::vector<Head> heads;
  long long replayed = 0, fused = 0, leg_pairs = 0;
  int status = 0;
};

static std::string num(double v)
{
  char s[64];
  snprintf(s, sizeof s, "%.17g", v);
  return s;
}

// B filters through the handlers; r / high: per-filter sweeps (setSweep) or empty, then the .cfg's r_cfg / high_cfg hold for every filter
static bool run(int n, int B, bool fuse, bool late, const std::vector<Tick> &log, const std::vector<double> &r, const std::vector<double> &high,
                double r_cfg, double high_cfg, const std::vector<int> &want, Run &out)
{
  double g;
  po_get_constants(&g, nullptr);
  BotParam param;
  param.set("state_estimator.utime_history_span", "1000000");
  param.set("state_estimator.history_slots", late ? "16" : "0");
  if (late) param.set("state_estimator.history_checkpoint_every", "1");
  param.set("state_estimator.fuse_ins_legodo", fuse ? "true" : "false");
  param.set("state_estimator.ins.channel", "IMU");
  param.set("state_estimator.ins.q_gyro", 0.5);
  param.set("state_estimator.ins.q_accel", 0.1);
  param.set("state_estimator.ins.timestep_dt", 0.002);
  param.set("state_estimator.ins.atlas_filter", "false");
  set_ins_bias_keys(param, n);
  param.applyOverrides("state_estimator.legodo.mode=lin_rate|state_estimator.legodo.r_xyz=2.0|state_estimator.legodo.r_vxyz=" + num(r_cfg) + "|"
                       "state_estimator.legodo.r_vang=3|state_estimator.legodo.r_vxyz_uncertain=14|state_estimator.legodo.r_vang_uncertain=9|"
                       "state_estimator.legodo.schmitt_low_threshold=475|state_estimator.legodo.schmitt_high_threshold=" + num(high_cfg) + "|"
                       "state_estimator.legodo.schmitt_low_delay=7000|state_estimator.legodo.schmitt_high_delay=7000|"
                       "state_estimator.legodo.filter_contact_events=true|state_estimator.legodo.zero_initial_velocity=3|"
                       "state_estimator.legodo.initialization_mode=zero|state_estimator.legodo.left_standing_link=l_foot|"
                       "state_estimator.legodo.right_standing_link=r_foot|state_estimator.legodo.filter_joint_positions=none|"
                       "state_estimator.legodo.total_force=900|state_estimator.legodo.standing_schmitt_level=0.65|"
                       "state_estimator.legodo.init_contact_mode=walking|state_estimator.legodo.use_controller_input=false|"
                       "state_estimator.legodo.torque_adjustment=true|state_estimator.legodo.adjustment_joints=l_leg_hpz,l_leg_kny,r_leg_kny|"
                       "state_estimator.legodo.adjustment_gain=7000,10000,10000");
  param.applyOverrides("state_estimator.fovis.mode=position_orient|state_estimator.fovis.r_pxyz=0.05|state_estimator.fovis.r_chi=0.05");
  for (const char *s : { "ins", "legodo", "fovis" }) {
    param.set(std::string("state_estimator.") + s + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + s + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + s + ".utime_offset", "0");
  }
  const std::vector<std::string> names = { "back_bkz", "l_leg_hpz", "l_leg_hpx", "l_leg_hpy", "neck_ay", "l_leg_kny", "l_leg_aky", "l_leg_akx",
                                           "l_arm_shz", "r_leg_hpz", "r_leg_hpx", "r_leg_hpy", "r_arm_shz", "r_leg_kny", "r_leg_aky", "r_leg_akx" };
  ModelClient model;
  if (!model.fromURDFString(URDF, "l_foot", "r_foot")) return false;
  RBIS x0(n, B);
  RBIM P0(n, B);
  for (int b = 0; b < B; b++) {   // every filter starts from the same state: they differ in the swept parameters alone
    double q[4];
    po_euler_to_quat(0.01, -0.02, 0.7, q);
    for (int i = 0; i < 4; i++) x0.q(i, b) = q[i];
    const double sig[15] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0 };
    for (int i = 0; i < 15; i++) P0(i, i, b) = sig[i] * sig[i];
    if (n == 21)
      for (int i = 0; i < 6; i++) {
        x0(15 + i, b) = (i < 3 ? 0.001 : 0.01) * (i - 2.5);
        P0(15 + i, 15 + i, b) = TEST_SIG_BIAS[i] * TEST_SIG_BIAS[i];
      }
  }
  BotTrans ins_to_body;
  InsHandler ins_handler(&param, &ins_to_body);
  FovisHandler fovis_handler(&param, 0);
  FrontEnd front_end(&param);
  auto on_ins = front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler);
  auto on_fovis = front_end.addSensor("fovis", &FovisHandler::processMessage, &fovis_handler);
  MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
  front_end.setStateEstimator(&est);
  {
    LegOdoHandler legodo_handler(&param, &model);
    if (!r.empty() && !legodo_handler.setSweep("state_estimator.legodo.r_vxyz", r)) return false;
    if (!high.empty() && !legodo_handler.setSweep("schmitt_high_threshold", high)) return false;
    auto on_joints = front_end.addSensor("legodo", &LegOdoHandler::processMessage, &legodo_handler);
    std::vector<double> vt(3 * (size_t) B), vq(4 * (size_t) B);
    for (int k = 0; k < T; k++) {
      const Tick &tk = log[k];
      const int64_t utime = 1000000 + (int64_t) (k + 1) * 2000;
      msgs::ins_t im{ utime, BatchArray(tk.imu, PB_HOST_BROADCAST), BatchArray(tk.imu + 3, PB_HOST_BROADCAST) };
      on_ins(&im);
      msgs::six_axis_force_torque_array_t ft{ utime, BatchArray(tk.fz, PB_HOST_BROADCAST) };
      legodo_handler.forceTorqueHandler(&ft, B);
      msgs::joint_state_t js;
      js.utime = utime;
      js.joint_name = names;
      js.joint_position = tk.jp;
      js.joint_effort = tk.je;
      js.joint_velocity = nullptr;
      js.mem = PB_HOST_BROADCAST;
      on_joints(&js);
      if (late && k % 10 == 9) {   // the VO message arrives behind the leg odometry it is older than; its keyframe is 8 ms back
        for (int b = 0; b < B; b++) {
          for (int i = 0; i < 3; i++) vt[(size_t) i * B + b] = tk.vo_t[i];
          for (int i = 0; i < 4; i++) vq[(size_t) i * B + b] = tk.vo_q[i];
        }
        msgs::update_t vo{ utime - 300, utime - 8300, nullptr, BatchArray(vt.data(), PB_HOST), BatchArray(vq.data(), PB_HOST) };
        on_fovis(&vo);
      }
    }
    est.flushPending();
  }
  RBIS head;
  RBIM cov;
  est.getHeadState(head, cov);
  const std::vector<double> ll = est.getMeasurementsLogLikelihood();
  for (int b : want) {
    Head h;
    for (int i = 0; i < n; i++) h.v.push_back(head(i, b));
    for (int i = 0; i < 4; i++) h.v.push_back(head.q(i, b));
    for (int c = 0; c < n; c++)
      for (int rr = 0; rr < n; rr++) h.v.push_back(cov(rr, c, b));
    h.v.push_back(ll[b]);
    out.heads.push_back(h);
  }
  out.replayed = est.replayed_updates;
  out.fused = est.fused_pairs;
  out.leg_pairs = est.leg_kernel_pairs;
  out.status = est.last_status;
  return true;
}

static int host_checks()
{
  BotParam param;
  param.applyOverrides("state_estimator.legodo.mode=lin_rate|state_estimator.legodo.r_xyz=0.2|state_estimator.legodo.r_vxyz=0.1|"
                       "state_estimator.legodo.r_vang=0.3|state_estimator.legodo.r_vxyz_uncertain=0.5|state_estimator.legodo.r_vang_uncertain=0.9");
  LegOdoHandler h(&param);
  int bad = 0;
  auto expect = [&](bool ok, const char *what) {
    if (!ok) { printf("FAIL: %s\n", what); bad = 1; }
  };
  const std::vector<double> v96(96, 1.0), v95(95, 1.0), none;
  expect(!h.setSweep("state_estimator.legodo.r_vxy", v96) && !h.setSweep("mode", v96) && !h.setSweep("", v96) && !h.sweep_dirty_ && h.sweep_B_ == 0,
         "an unknown key is refused and changes nothing");
  expect(!h.setSweep("r_vxyz", none) && h.sweep_B_ == 0, "an empty sweep is refused");
  const char *keys[11] = { "r_vxyz", "r_vxyz_uncertain", "r_vang", "r_vang_uncertain", "r_xyz", "schmitt_low_threshold", "schmitt_high_threshold",
                           "schmitt_low_delay", "schmitt_high_delay", "total_force", "standing_schmitt_level" };
  for (int i = 0; i < 11; i++) {
    LegOdoHandler hk(&param);
    expect(hk.setSweep(std::string(i % 2 ? "state_estimator.legodo." : "") + keys[i], v96) && hk.sweep_rows_[i].size() == 96 && hk.sweep_dirty_, keys[i]);
  }
  expect(h.setSweep("r_vxyz", v96) && h.sweep_B_ == 96 && h.sweep_rows_[PB_LEGPAR_R_VXYZ].size() == 96, "the first sweep fixes the batch size");
  expect(!h.setSweep("schmitt_high_threshold", v95) && h.sweep_rows_[PB_LEGPAR_SCHMITT_HIGH].empty() && h.sweep_B_ == 96,
         "another length is refused and changes nothing");
  expect(!h.setSweep("r_vxyz", v95) && h.sweep_rows_[PB_LEGPAR_R_VXYZ].size() == 96, "... also for a key that was swept before");
  printf(bad ? "FAIL\n" : "PASS\n");
  return bad;
}

int main(int argc, char **argv)
{
  const int n = take_n_states(argc, argv);
  const std::string what = argc > 1 ? argv[1] : "fuse";
  if (what == "host") return host_checks();
  const bool fuse = what == "fuse", late = argc > 2 && std::string(argv[2]) == "late";
  double g;
  po_get_constants(&g, nullptr);
  std::vector<Tick> log(T);
  const double period = 1.1, phase = 0.15, swing = 0.25;
  for (int k = 0; k < T; k++) {
    Tick &tk = log[k];
    const double t = (k + 1) * 0.002;
    const double v[6] = { 0.2 * sin(0.05 * k), 0.05, -0.1 * cos(0.03 * k), 0.3 * nrand(), 0.3 * nrand(), g + 0.3 * nrand() };
    for (int i = 0; i < 6; i++) tk.imu[i] = v[i];
    double ph = t / period + phase;
    ph -= floor(ph);
    double wl = ramp(ph) * ramp(0.6 - ph), wr = ramp(ph - 0.5) * ramp(1.1 - ph) + (ph < 0.1 ? ramp(0.1 - ph) : 0.0);
    if (t < 0.4) wl = wr = 1.0;
    tk.fz[0] = -(900 * wl + 5 * nrand());
    tk.fz[1] = 900 * wr + 5 * nrand();
    const double sw = sin(2 * M_PI * ph);
    for (int j = 0; j < NJ; j++) { tk.jp[j] = (float) (0.3 * nrand()); tk.je[j] = (float) (40 * nrand()); }
    for (int side = 0; side < 2; side++) {
      const double sgn = side ? -1.0 : 1.0, lift = fmax(0.0, -sgn * sw);
      const int r0 = side ? 9 : 1, r1 = side ? 13 : 5;
      tk.jp[r0 + 0] = (float) (0.05 * sgn * sw);
      tk.jp[r0 + 1] = (float) (0.03 * sgn + 0.02 * sw);
      tk.jp[r0 + 2] = (float) (-0.35 - sgn * swing * sw - 0.2 * lift);
      tk.jp[r1 + 0] = (float) (0.7 + 0.5 * lift);
      tk.jp[r1 + 1] = (float) (-0.35 + sgn * swing * sw * 0.5 - 0.3 * lift);
      tk.jp[r1 + 2] = (float) (-0.03 * sgn - 0.02 * sw);
    }
    for (int i = 0; i < 3; i++) tk.vo_t[i] = 0.004 * nrand();
    po_euler_to_quat(0.002 * nrand(), 0.002 * nrand(), 0.004 * nrand(), tk.vo_q);
  }
  const int B = 96;
  std::vector<double> r(B), high(B);
  for (int b = 0; b < B; b++) {
    r[b] = 5.0 + 7.0 * b / (B - 1);            // r_vxyz 5 ... 12 m/s (tests/test_leg_odometry.py R_VXYZ: not below 5)
    high[b] = 520.0 + 180.0 * b / (B - 1);     // schmitt_high_threshold 520 ... 700 N
  }
  const std::vector<int> pick = { 0, 47, 95 };
  Run sweep;
  if (!run(n, B, fuse, late, log, r, high, 0.1, 525.0, pick, sweep)) { printf("FAIL: the sweep did not run\n"); return 1; }
  double worst = 0;
  bool ok = sweep.status == PB_OK, bits = true, apart = false;
  for (size_t i = 0; i < pick.size(); i++) {
    Run one;
    if (!run(n, 1, fuse, late, log, {}, {}, r[pick[i]], high[pick[i]], { 0 }, one)) { printf("FAIL: the single run did not run\n"); return 1; }
    const std::vector<double> &a = sweep.heads[i].v, &c = one.heads[0].v;
    // relative to the largest entry of each block: vec | quat | cov | ll
    const size_t cut[5] = { 0, (size_t) n, (size_t) n + 4, (size_t) n + 4 + (size_t) n * n, a.size() };
    double rel = 0;
    for (int blk = 0; blk < 4; blk++) {
      double e = 0, s = 1e-300;
      for (size_t j = cut[blk]; j < cut[blk + 1]; j++) { e = fmax(e, fabs(a[j] - c[j])); s = fmax(s, fabs(c[j])); if (!std::isfinite(a[j])) ok = false; }
      rel = fmax(rel, e / s);
    }
    bits = bits && memcmp(a.data(), c.data(), sizeof(double) * a.size()) == 0;
    worst = fmax(worst, rel);
    ok = ok && one.status == PB_OK && (!late || one.replayed > 0);
    printf("filter %2d (r_vxyz %.4f, schmitt_high_threshold %.2f) against a batch of one: rel err %.2e\n", pick[i], r[pick[i]], high[pick[i]], rel);
    if (i > 0) apart = apart || memcmp(sweep.heads[i].v.data(), sweep.heads[0].v.data(), sizeof(double) * a.size()) != 0;
  }
  printf("n=%d %s%s: worst rel err %.2e, bit-equal: %s; fused pairs %lld (inside the pair kernel %lld), updates re-applied after late arrivals %lld\n", n,
         fuse ? "fused" : "not fused", late ? ", late VO" : "", worst, bits ? "yes" : "no", sweep.fused, sweep.leg_pairs, sweep.replayed);
  ok = ok && worst < 1e-12 && apart /* the swept values reach the filters */ && (!late || sweep.replayed > 0) && (!fuse || sweep.leg_pairs > T / 2);
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
