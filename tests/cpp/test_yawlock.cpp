// test_yawlock.cpp -- a miniature se-fusion with active_sensors = [ins, legodo, yawlock] (fusion.cpp:233-241): InsHandler,
// LegOdoHandler and YawLockHandler on one joint-state channel, the status channel named by state_estimator.yawlock.behavior_channel
// (both message types also go through their wire encoding), and a scan-match pose every 40 ticks.
//   argv[1]: dump file     argv[2]: yaw-lock mode (yawbias | yaw | yawbias_yaw | anything else = the reference's fallback to yaw)
//   argv[3]: ctrl | ihmc   "n21" anywhere: the 21-state filter
// Run 1 (in order) writes per joint-state message what tests/test_yawlock_shim.py needs to hold the handler against the numpy
// restatement of the reference and the oracle's update: the raw status event, the gyro sample, the joint positions, every filter's
// head in front of the yaw-lock update, its yaw-lock state behind it, and -- on sampled messages -- the full prior and posterior.
// Run 2 delivers every pose 7 ticks LATE (posterior checkpoints on): the replay crosses yaw-lock updates, must re-apply their kept
// measurements, and must end where run 1 ends with the same yaw-lock state (counter included: pb_yawlock_get).
// Exit code 0 + "PASS".  Needs a GPU.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "test_n.hpp"

using namespace MavStateEst;

static uint64_t rng_state;
static double urand()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }

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

static const int B = 8, T = 900, NJ = 16, DT_US = 5000, PERIOD = 7;

struct Result {
  std::vector<double> vec, quat, cov;
  std::vector<int64_t> info;
  int64_t replayed = 0, idle = 0;
};

static bool run(int n, const std::string &mode, bool ihmc, bool late, FILE *dump, Result &out)
{
  rng_state = 0x59414c4f434bULL;
  double g;
  po_get_constants(&g, nullptr);
  BotParam param;
  param.set("state_estimator.utime_history_span", "1000000");
  param.set("state_estimator.history_slots", "40");
  param.set("state_estimator.history_checkpoint_every", "1");
  param.set("state_estimator.ins.channel", "IMU");
  param.set("state_estimator.ins.q_gyro", 0.5);
  param.set("state_estimator.ins.q_accel", 0.1);
  param.set("state_estimator.ins.timestep_dt", 0.005);
  param.set("state_estimator.ins.atlas_filter", "false");
  set_ins_bias_keys(param, n);
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
  // the hold-off after a slip comes from yaw_slip_threshold_degrees as well (rbis_yawlock_update.cpp:19): 0.4 s here
  param.applyOverrides(std::string("state_estimator.yawlock.correction_period=") + std::to_string(PERIOD) +
                       "|state_estimator.yawlock.yaw_slip_detect=true|state_estimator.yawlock.yaw_slip_threshold_degrees=0.4|"
                       "state_estimator.yawlock.behavior_channel=" + (ihmc ? "ROBOT_BEHAVIOR" : "CONTROLLER_STATUS") +
                       "|state_estimator.yawlock.mode=" + mode + "|state_estimator.yawlock.r_yaw_bias=0.05|state_estimator.yawlock.r_yaw=1.0");
  for (const char *s : { "ins", "legodo", "yawlock", "scan_matcher" }) {
    param.set(std::string("state_estimator.") + s + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + s + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + s + ".utime_offset", "0");
  }
  // The handler forms its measurement from the head at the moment the message is processed, in the reference as here, so a late
  // measurement that MOVES the head makes the delayed run differ from the in-order one by construction.  The pose therefore
  // carries no information (R of 1e8 m / 1e8 deg: its gain is below rounding): the replay machinery runs in full -- restore the
  // checkpoint, re-apply everything behind it, yaw-lock updates included -- and "equals the in-order run" is an exact statement.
  param.applyOverrides("state_estimator.scan_matcher.mode=position_yaw|state_estimator.scan_matcher.r_pxy=1e8|"
                       "state_estimator.scan_matcher.r_pz=1e8|state_estimator.scan_matcher.r_yaw=1e8");
  const std::vector<std::string> names = { "back_bkz", "l_leg_hpz", "l_leg_hpx", "l_leg_hpy", "neck_ay", "l_leg_kny", "l_leg_aky", "l_leg_akx",
                                           "l_arm_shz", "r_leg_hpz", "r_leg_hpx", "r_leg_hpy", "r_arm_shz", "r_leg_kny", "r_leg_aky", "r_leg_akx" };
  ModelClient model;
  if (!model.fromURDFString(URDF, "l_foot", "r_foot")) { printf("FAIL: URDF chains\n"); return false; }
  RBIS x0(n, B);
  RBIM P0(n, B);
  for (int b = 0; b < B; b++) {
    double q[4];
    po_euler_to_quat(0.04 * (urand() - 0.5), 0.04 * (urand() - 0.5), 0.6 * (urand() - 0.5), q);
    for (int i = 0; i < 4; i++) x0.q(i, b) = q[i];
    const double sig[15] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0 };
    for (int i = 0; i < 15; i++) P0(i, i, b) = sig[i] * sig[i];
    po_rbis ox;
    po_rbim oP;
    po_rbis_zero(&ox);
    memset(&oP, 0, sizeof oP);
    init_bias_states(n, b, x0, P0, &ox, &oP, urand);
  }
  // an IMU that is not aligned with the body: insHandler must rotate the gyro (rbis_yawlock_update.cpp:113)
  BotTrans ins_to_body;
  po_euler_to_quat(0.0, 0.0, M_PI / 2, ins_to_body.rot_quat);
  InsHandler ins_handler(&param, &ins_to_body);
  ScanMatcherHandler sm_handler(&param);
  LegOdoHandler legodo_handler(&param, &model);
  YawLockHandler yaw_handler(&param, &model, &ins_to_body);
  const int want_mode = mode == "yawbias" ? 0 : (mode == "yawbias_yaw" ? 2 : 1);
  if ((int) yaw_handler.mode != want_mode || yaw_handler.yaw_slip_disable_period != 0.4) { printf("FAIL: YawLockHandler configuration\n"); return false; }
  FrontEnd front_end(&param);
  auto on_ins = front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler);
  auto on_pose = front_end.addSensor("scan_matcher", &ScanMatcherHandler::processMessage, &sm_handler);
  auto on_legodo = front_end.addSensor("legodo", &LegOdoHandler::processMessage, &legodo_handler);
  auto on_yawlock = front_end.addSensor("yawlock", &YawLockHandler::processMessage, &yaw_handler);
  MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
  front_end.setStateEstimator(&est);
  std::vector<float> jp(NJ), base(NJ);
  for (int j = 0; j < NJ; j++) base[j] = (float) (0.3 * nrand());
  for (int side = 0; side < 2; side++) {
    const double sgn = side ? -1.0 : 1.0;
    const int r0 = side ? 9 : 1, r1 = side ? 13 : 5;
    base[r0] = (float) (0.05 * sgn); base[r0 + 1] = (float) (0.03 * sgn); base[r0 + 2] = -0.35f;
    base[r1] = 0.7f; base[r1 + 1] = -0.35f; base[r1 + 2] = (float) (-0.03 * sgn);
  }
  struct Pending { int due; int64_t utime; double pos[3], quat[4]; };
  std::vector<Pending> pending;
  RBIS hs(n, B), hs2(n, B);
  RBIM hc(n, B), hc2(n, B);
  const double zero3[3] = { 0, 0, 0 }, fz[2] = { -450.0, 455.0 };
  for (int k = 0; k < T; k++) {
    const int64_t utime = 1000000 + (int64_t) (k + 1) * DT_US;
    const double t = (k + 1) * DT_US * 1e-6;
    // ---- status channel, every 100 ticks, through the wire image ----
    double ev[3] = { 0, 0, 0 };
    if (k % 100 == 0) {
      std::vector<uint8_t> buf;
      if (ihmc) {   // walks until 0.5 s, then "stands": the 3-second rule keeps the lock off until 3.5 s
        pronto_wire::behavior_t w, r;
        w.utime = utime;
        w.behavior = k < 100 ? pronto_wire::behavior_t::BEHAVIOR_WALK : (k == 500 ? pronto_wire::behavior_t::BEHAVIOR_MANIPULATE : pronto_wire::behavior_t::BEHAVIOR_STAND);
        w.encode(buf);
        if (r.decode(buf.data(), buf.size()) != (int) buf.size() || buf.size() != 20) { printf("FAIL: behavior_t wire image\n"); return false; }
        msgs::behavior_t m;
        m.utime = r.utime; m.behavior = r.behavior;
        yaw_handler.robotBehaviorHandler(&m);
        ev[0] = 2; ev[1] = r.behavior; ev[2] = (double) r.utime;
      } else {      // unknown, standing, walking for a while, manipulating, standing
        const int8_t seq[9] = { 0, 1, 1, 1, 2, 8, 1, 1, 1 };
        pronto_wire::controller_status_t w, r;
        w.utime = utime; w.state = seq[k / 100]; w.controller_utime = utime - 7; w.V = 0.5f; w.Vdot = -0.25f;
        w.encode(buf);
        if (r.decode(buf.data(), buf.size()) != (int) buf.size() || buf.size() != 33 || r.V != 0.5f || r.controller_utime != utime - 7) { printf("FAIL: controller_status_t wire image\n"); return false; }
        msgs::controller_status_t m;
        m.utime = r.utime; m.state = r.state;
        yaw_handler.controllerStatusHandler(&m);
        ev[0] = 1; ev[1] = r.state; ev[2] = (double) r.utime;
      }
    }
    // ---- IMU ----
    const double v[6] = { 0.02 * sin(0.05 * k), 0.01 * nrand(), 0.03 * cos(0.03 * k), 0.2 * nrand(), 0.2 * nrand(), g + 0.2 * nrand() };
    msgs::ins_t im{ utime, BatchArray(v, PB_HOST_BROADCAST), BatchArray(v + 3, PB_HOST_BROADCAST) };
    yaw_handler.insHandler(&im);
    on_ins(&im);
    // ---- late poses that have come due ----
    for (size_t i = 0; i < pending.size();)
      if (pending[i].due == k) {
        msgs::pose_t pm{ pending[i].utime, BatchArray(pending[i].pos, PB_HOST_BROADCAST), BatchArray(zero3, PB_HOST_BROADCAST), BatchArray(pending[i].quat, PB_HOST_BROADCAST) };
        on_pose(&pm);
        pending.erase(pending.begin() + (long) i);
      } else i++;
    // ---- joint state: a standing robot that sways; at tick 800 the left hip yaw turns by 1 degree (a slip, threshold 0.4) ----
    for (int j = 0; j < NJ; j++) jp[j] = base[j];
    jp[3] += (float) (0.02 * sin(1.3 * t)); jp[11] += (float) (0.02 * sin(1.3 * t));
    jp[5] -= (float) (0.02 * sin(1.3 * t)); jp[13] -= (float) (0.02 * sin(1.3 * t));
    if (k >= 800) jp[1] += (float) (M_PI / 180.0);
    msgs::six_axis_force_torque_array_t ft{ utime, BatchArray(fz, PB_HOST_BROADCAST) };
    legodo_handler.forceTorqueHandler(&ft, B);
    msgs::joint_state_t js;
    js.utime = utime;
    js.joint_name = names;
    js.joint_position = jp.data();
    js.mem = PB_HOST_BROADCAST;
    on_legodo(&js);
    const bool full = dump && (k % PERIOD == 0 || k % 10 == 3);
    if (dump) est.getHeadState(hs, hc);
    on_yawlock(&js);
    if (dump) {
      est.getHeadState(hs2, hc2);
      std::vector<double> rec = { (double) k, (double) utime, ev[0], ev[1], ev[2], yaw_handler.body_gyro[2], full ? 1.0 : 0.0 };
      for (int j = 0; j < NJ; j++) rec.push_back(jp[j]);
      for (int b = 0; b < B; b++) {
        for (int i = 0; i < 3; i++) rec.push_back(hs(9 + i, b));
        for (int i = 0; i < 4; i++) rec.push_back(hs.q(i, b));
        rec.push_back(n == 21 ? hs(17, b) : 0.0);
        double poses[14];
        int64_t info[4];
        if (pb_yawlock_get(est.ctx, b, poses, info) != PB_OK) { printf("FAIL: pb_yawlock_get\n"); return false; }
        for (int i = 0; i < 4; i++) rec.push_back((double) info[i]);
      }
      if (full)
        for (int which = 0; which < 2; which++) {
          const RBIS &s = which ? hs2 : hs;
          const RBIM &c = which ? hc2 : hc;
          for (int b = 0; b < B; b++) {
            for (int i = 0; i < n; i++) rec.push_back(s(i, b));
            for (int i = 0; i < 4; i++) rec.push_back(s.q(i, b));
            for (int r = 0; r < n; r++)
              for (int cc = 0; cc < n; cc++) rec.push_back(c(r, cc, b));
          }
        }
      fwrite(rec.data(), sizeof(double), rec.size(), dump);
    }
    // ---- scan-match pose every 40 ticks, stamped between this tick and the next; run 2 delivers it 7 ticks late ----
    if (k % 40 == 20) {
      Pending p;
      p.due = k + 7;
      p.utime = utime + 1000;
      for (int i = 0; i < 3; i++) p.pos[i] = 0.05 * nrand();
      po_euler_to_quat(0.0, 0.0, 0.1 * (urand() - 0.5), p.quat);
      if (late) pending.push_back(p);
      else {
        msgs::pose_t pm{ p.utime, BatchArray(p.pos, PB_HOST_BROADCAST), BatchArray(zero3, PB_HOST_BROADCAST), BatchArray(p.quat, PB_HOST_BROADCAST) };
        on_pose(&pm);
      }
    }
  }
  if (est.last_status != PB_OK) { printf("FAIL: estimator status %d: %s\n", est.last_status, pb_last_error(est.ctx)); return false; }
  est.getHeadState(hs, hc);
  out.vec = hs.vec; out.quat = hs.quat; out.cov = hc.m;
  out.info.resize(4 * B);
  double poses[14];
  for (int b = 0; b < B; b++)
    if (pb_yawlock_get(est.ctx, b, poses, &out.info[4 * (size_t) b]) != PB_OK) return false;
  out.replayed = est.replayed_updates;
  return true;
}

static double rel(const std::vector<double> &a, const std::vector<double> &b)
{
  double d = 0, s = 1e-300;
  for (size_t i = 0; i < a.size(); i++) { d = fmax(d, fabs(a[i] - b[i])); s = fmax(s, fabs(b[i])); }
  return d / s;
}

int main(int argc, char **argv)
{
  const int n = take_n_states(argc, argv);
  if (argc < 4) { printf("usage: test_yawlock <dump> <mode> ctrl|ihmc [n21]\n"); return 2; }
  const std::string mode = argv[2];
  const bool ihmc = std::string(argv[3]) == "ihmc";
  {  // insHandler applies the ins_to_body rotation (rbis_yawlock_update.cpp:113): a roll of +90 degrees takes gyro y to body z
    BotParam p;
    p.applyOverrides("state_estimator.yawlock.correction_period=1|state_estimator.yawlock.yaw_slip_detect=false|"
                     "state_estimator.yawlock.yaw_slip_threshold_degrees=1|state_estimator.yawlock.behavior_channel=ROBOT_BEHAVIOR|"
                     "state_estimator.yawlock.mode=yaw|state_estimator.yawlock.r_yaw=1|state_estimator.legodo.left_standing_link=l_foot|"
                     "state_estimator.legodo.right_standing_link=r_foot");
    BotTrans roll;
    po_euler_to_quat(M_PI / 2, 0.0, 0.0, roll.rot_quat);
    YawLockHandler h(&p, nullptr, &roll);
    const double gy[3] = { 0.1, 0.2, 0.3 }, zero[3] = { 0, 0, 0 };
    msgs::ins_t im{ 1, BatchArray(gy, PB_HOST_BROADCAST), BatchArray(zero, PB_HOST_BROADCAST) };
    h.insHandler(&im);
    if (fabs(h.body_gyro[2] - 0.2) > 1e-15 || fabs(h.body_gyro[1] + 0.3) > 1e-15) { printf("FAIL: insHandler rotation\n"); return 1; }
  }
  FILE *dump = fopen(argv[1], "wb");
  if (!dump) { printf("FAIL: cannot write %s\n", argv[1]); return 1; }
  Result in_order, replayed;
  const bool ok1 = run(n, mode, ihmc, false, dump, in_order);
  fclose(dump);
  if (!ok1 || !run(n, mode, ihmc, true, nullptr, replayed)) return 1;
  const double ev = rel(replayed.vec, in_order.vec), eq = rel(replayed.quat, in_order.quat), ec = rel(replayed.cov, in_order.cov);
  printf("B=%d T=%d n=%d mode=%s: replay vs in order: vec %.3g quat %.3g cov %.3g; %" PRId64 " updates re-applied; counter %" PRId64 "\n", B, T, n,
         mode.c_str(), ev, eq, ec, replayed.replayed, in_order.info[0]);
  if (replayed.replayed < 100 || in_order.replayed != 0) { printf("FAIL: the late poses forced no replay\n"); return 1; }
  if (replayed.info != in_order.info) { printf("FAIL: the replay changed the yaw-lock state (it must not run the state machine again)\n"); return 1; }
  if (mode != "yawbias" && in_order.info[0] != T) { printf("FAIL: counter %" PRId64 " after %d messages\n", in_order.info[0], T); return 1; }
  if (!(ev <= 1e-12 && eq <= 1e-12 && ec <= 1e-12)) { printf("FAIL: the replay does not end where the in-order run ends\n"); return 1; }
  printf("PASS\n");
  return 0;
}
