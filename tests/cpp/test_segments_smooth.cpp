// test_segments_smooth.cpp -- whole-log RTS smoothing of N independent log segments as ONE batch (SegmentBatcher::enableSmoothing /
// smooth, pronto_amd/csrc/segment_batcher.hpp): the reference's "-S" run (lcm_front_end.cpp:168-203, mav_state_est.cpp:98-189) of every
// log of se-batch-process.sh (motion_estimate/scripts/se-batch-process.sh:17-26,58-74), with every log its own length.
//   * 64 DIFFERENT synthetic logs (LogWriter): another gait, IMU stream, absolute time base and time-stamp jitter per log, lengths that
//     differ by up to 40 %; channels IMU (bot_core::ins_t), FORCE_TORQUE, JOINT_STATE, POSE_SCAN, replayed through InsHandler,
//     LegOdoHandler (lin_rate, torque adjustment, contact logic) and ScanMatcherHandler (position_yaw);
//   (a) every segment's smoothed posteriors (emit mask), their count, order and message times equal a B = 1 run of that log alone
//       through the same handlers and the two-argument EKFSmoothBackwardsPass, <= 1e-9 block-relative;
//   (b) segments 0, 1, 7 and 8 also equal the oracle directly: the single-segment forward run (po_imu_process_step, po_torque_adjust ->
//       po_fk -> po_leg_update_wc -> po_indexed_update, po_indexed_orient_update) and the backward recursion with po_ekf_smoothing_step;
//   (c) with every log of the same length, smooth() is bit for bit the two-argument pass and launches no select (smoother_masked_steps 0);
//   (d) at and after a segment's last INS update its rows hold its final posterior (the terminal slot, carried by the masked steps) bit
//       for bit, while the two-argument pass leaves the idle state there: not bit for bit the final posterior, for every segment that ends
//       early (asserted; on these logs the difference is at rounding level, ~1e-20 relative, in the angular-velocity / acceleration
//       entries the idle steps re-derive).  Its emitted rows are printed only: they agree with (a) to rounding here, since an idle tick's
//       predicted and carried states are the same idle state.
// Segment 0 ends before segment 5, so the lead segment (whose times the batched messages carry) changes mid-run.
// argv: "n21" = 21 states, "nofuse" = without fuse_ins_legodo, "every=K" = history_checkpoint_every, "time" = also time smooth() against
// 64 sequential single-segment passes, a directory for the logs.  Exit code 0 + "PASS".  Needs a GPU.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "test_n.hpp"
#include "../../pronto_amd/csrc/segment_batcher.hpp"

using namespace MavStateEst;

static uint64_t rng_state = 0x534d4f4fULL;
static double urand()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }
static double ramp(double x) { return x < 0 ? 0 : (x > 0.05 ? 1.0 : x / 0.05); }

static const char *URDF = R"(<robot name="biped">
  <joint name="l_leg_hpz" type="revolute"><origin xyz="0 0.089 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="l_uglut"/></joint>
  <joint name="l_leg_hpx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="l_uglut"/><child link="l_lglut"/></joint>
  <joint name="l_leg_hpy" type="revolute"><origin xyz="0.05 0.0225 -0.066"/><axis xyz="0 1 0"/><parent link="l_lglut"/><child link="l_uleg"/></joint>
  <joint name="l_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374" rpy="0 0.02 0"/><axis xyz="0 1 0"/><parent link="l_uleg"/><child link="l_lleg"/></joint>
  <joint name="l_leg_aky" type="revolute"><origin xyz="0 0 -0.422"/><axis xyz="0 1 0"/><parent link="l_lleg"/><child link="l_talus"/></joint>
  <joint name="l_leg_akx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="l_talus"/><child link="l_foot"/></joint>
  <joint name="r_leg_hpz" type="revolute"><origin xyz="0 -0.089 0"/><axis xyz="0 0 1"/><parent link="pelvis"/><child link="r_uglut"/></joint>
  <joint name="r_leg_hpx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="r_uglut"/><child link="r_lglut"/></joint>
  <joint name="r_leg_hpy" type="revolute"><origin xyz="0.05 -0.0225 -0.066"/><axis xyz="0 1 0"/><parent link="r_lglut"/><child link="r_uleg"/></joint>
  <joint name="r_leg_kny" type="revolute"><origin xyz="-0.05 0 -0.374" rpy="0 0.02 0"/><axis xyz="0 1 0"/><parent link="r_uleg"/><child link="r_lleg"/></joint>
  <joint name="r_leg_aky" type="revolute"><origin xyz="0 0 -0.422"/><axis xyz="0 1 0"/><parent link="r_lleg"/><child link="r_talus"/></joint>
  <joint name="r_leg_akx" type="revolute"><origin xyz="0 0 0"/><axis xyz="1 0 0"/><parent link="r_talus"/><child link="r_foot"/></joint>
</robot>)";

static const char *BOT_CORE_LCM = R"(package bot_core;
struct ins_t { int64_t utime; int64_t device_time; double gyro[3]; double mag[3]; double accel[3]; double quat[4]; double pressure; double rel_alt; }
struct joint_state_t { int64_t utime; int16_t num_joints; string joint_name[num_joints]; float joint_position[num_joints];
  float joint_velocity[num_joints]; float joint_effort[num_joints]; }
struct six_axis_force_torque_t { int64_t utime; double force[3]; double moment[3]; }
struct six_axis_force_torque_array_t { int64_t utime; int32_t num_sensors; string names[num_sensors]; six_axis_force_torque_t sensors[num_sensors]; }
struct pose_t { int64_t utime; double pos[3]; double vel[3]; double orientation[4]; double rotation_rate[3]; double accel[3]; }
)";

static const int NSEG = 64, T_MAX = 160, NJ = 16;
static const double SMOOTH_DT = 0.002;
static const std::vector<std::string> JOINTS = { "back_bkz", "l_leg_hpz", "l_leg_hpx", "l_leg_hpy", "neck_ay", "l_leg_kny", "l_leg_aky", "l_leg_akx",
                                                  "l_arm_shz", "r_leg_hpz", "r_leg_hpx", "r_leg_hpy", "r_arm_shz", "r_leg_kny", "r_leg_aky", "r_leg_akx" };

struct Tick {   // one tick of one log, as the oracle replays it
  int64_t imu_utime, js_utime;
  double gyro[3], accel[3], fz[2];
  float jp[NJ], je[NJ];
  bool pose;
  double pos[3], quat[4];
};

// ragged: up to 40 % shorter logs; else every log has the length of the shortest ragged one
static bool write_logs(const std::string &dir, const char *tag, bool ragged, double g, const pronto_wire::Schema &schema,
                       std::vector<std::vector<Tick>> &ticks, std::vector<std::string> &paths)
{
  rng_state = 0x534d4f4fULL;
  ticks.assign(NSEG, {});
  paths.assign(NSEG, "");
  for (int s = 0; s < NSEG; s++) {
    // (segment 0 is not the longest: the lead -- the lowest-numbered segment with events left -- changes from 0 to 5 mid-run)
    const int Ts = ragged ? T_MAX - ((s + 4) % 9) * 8 : T_MAX - 64;
    const int64_t base = 1000000000LL * (s + 1) + 7919 * s;   // another absolute time base per recording
    const double period = 0.7 + 0.6 * urand(), phase = urand(), swing = 0.1 + 0.25 * urand(), jit = 20 + 60 * urand();
    paths[(size_t) s] = dir + "/smooth_" + tag + "_" + std::to_string(s) + ".lcmlog";
    pronto_wire::LogWriter log(paths[(size_t) s]);
    if (!log.good()) return false;
    ticks[(size_t) s].resize((size_t) Ts);
    for (int k = 0; k < Ts; k++) {
      Tick &tk = ticks[(size_t) s][(size_t) k];
      const int64_t nominal = base + (int64_t) (k + 1) * 2000;
      tk.imu_utime = nominal + (int64_t) (jit * (urand() - 0.5));
      tk.js_utime = nominal + 300 + (int64_t) (jit * (urand() - 0.5));
      const double t = (k + 1) * 0.002;
      for (int i = 0; i < 3; i++) tk.gyro[i] = 0.2 * sin(0.05 * k + s + i) + 0.01 * nrand();
      for (int i = 0; i < 3; i++) tk.accel[i] = 0.3 * nrand() + (i == 2 ? g : 0.0);
      double ph = t / period + phase;
      ph -= floor(ph);
      double wl = ramp(ph) * ramp(0.6 - ph), wr = ramp(ph - 0.5) * ramp(1.1 - ph) + (ph < 0.1 ? ramp(0.1 - ph) : 0.0);
      if (t < 0.1) wl = wr = 1.0;
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
      tk.pose = (k % 20 == 19);
      for (int i = 0; i < 3; i++) tk.pos[i] = 0.05 * nrand();
      po_euler_to_quat(0.0, 0.0, 0.3 * (urand() - 0.5), tk.quat);
      pronto_wire::Writer w;
      w.u64(schema.fingerprint("bot_core.ins_t"));
      w.i64(tk.imu_utime); w.i64(tk.imu_utime + 17);
      w.f64s(tk.gyro, 3);
      for (int i = 0; i < 3; i++) w.f64(0.1 * i);
      w.f64s(tk.accel, 3);
      for (int i = 0; i < 4; i++) w.f64(i == 0);
      w.f64(1013.0); w.f64(0.0);
      log.write(tk.imu_utime, "IMU", w.buf);
      pronto_wire::Writer f;
      f.u64(schema.fingerprint("bot_core.six_axis_force_torque_array_t"));
      f.i64(tk.imu_utime + 100); f.i32(2); f.str("l_foot"); f.str("r_foot");
      for (int k2 = 0; k2 < 2; k2++) {
        f.i64(tk.imu_utime + 100);
        f.f64(1.0); f.f64(-2.0); f.f64(tk.fz[k2]);
        f.f64(0.1); f.f64(0.2); f.f64(0.3);
      }
      log.write(tk.imu_utime + 100, "FORCE_TORQUE", f.buf);
      pronto_wire::Writer j;
      j.u64(schema.fingerprint("bot_core.joint_state_t"));
      j.i64(tk.js_utime); j.i16((int16_t) NJ);
      for (int q = 0; q < NJ; q++) j.str(JOINTS[(size_t) q]);
      for (int q = 0; q < NJ; q++) j.f32(tk.jp[q]);
      for (int q = 0; q < NJ; q++) j.f32(0.0f);
      for (int q = 0; q < NJ; q++) j.f32(tk.je[q]);
      log.write(tk.js_utime, "JOINT_STATE", j.buf);
      if (tk.pose) {
        pronto_wire::Writer p;
        p.u64(schema.fingerprint("bot_core.pose_t"));
        p.i64(tk.js_utime + 200);
        p.f64s(tk.pos, 3);
        for (int i = 0; i < 3; i++) p.f64(0.0);
        p.f64s(tk.quat, 4);
        for (int i = 0; i < 6; i++) p.f64(0.0);
        log.write(tk.js_utime + 200, "POSE_SCAN", p.buf);
      }
    }
  }
  return true;
}

// one sink / callback call: the slot's posteriors of every filter of the run (getHeadState layout: [n][B], [4][B], [n][n][B])
struct Call {
  int step = -1;
  int64_t utime = 0;
  std::vector<uint8_t> emit;
  std::vector<int64_t> utimes;
  std::vector<double> vec, quat, cov;
};
struct Out {
  int ret = -2, status = PB_OK, B = 0;
  int64_t masked = 0, fused = 0, reapplied = 0;
  double sec = 0;   // wall time of the backward pass (with read = false: nothing read back)
  std::vector<Call> calls;
  Call final_;   // smooth: finalState(), every segment's head at the end of its own log
};

struct Setup {
  int n;
  bool fuse;
  int every;
  const pronto_wire::Schema *schema;
  RBIS x0;
  RBIM P0;
};

static void set_params(BotParam &param, const Setup &su)
{
  const int n = su.n;
  param.set("state_estimator.utime_history_span", "100000000");
  param.set("state_estimator.history_slots", (double) (3 * T_MAX + 40));
  param.set("state_estimator.history_checkpoint_every", (double) su.every);
  param.set("state_estimator.fuse_ins_legodo", su.fuse ? "true" : "false");
  param.set("state_estimator.ins.channel", "IMU");
  param.set("state_estimator.ins.q_gyro", 0.5);
  param.set("state_estimator.ins.q_accel", 0.1);
  param.set("state_estimator.ins.timestep_dt", 0.002);
  param.set("state_estimator.ins.atlas_filter", "false");
  set_ins_bias_keys(param, n);
  param.applyOverrides("state_estimator.legodo.mode=lin_rate|state_estimator.legodo.r_xyz=2.0|state_estimator.legodo.r_vxyz=5|"
                       "state_estimator.legodo.r_vang=3|state_estimator.legodo.r_vxyz_uncertain=10|state_estimator.legodo.r_vang_uncertain=9|"
                       "state_estimator.legodo.schmitt_low_threshold=475|state_estimator.legodo.schmitt_high_threshold=525|"
                       "state_estimator.legodo.schmitt_low_delay=7000|state_estimator.legodo.schmitt_high_delay=7000|"
                       "state_estimator.legodo.filter_contact_events=true|state_estimator.legodo.zero_initial_velocity=3|"
                       "state_estimator.legodo.initialization_mode=zero|state_estimator.legodo.left_standing_link=l_foot|"
                       "state_estimator.legodo.right_standing_link=r_foot|state_estimator.legodo.filter_joint_positions=none|"
                       "state_estimator.legodo.init_contact_mode=walking|state_estimator.legodo.use_controller_input=false|"
                       "state_estimator.legodo.total_force=900|state_estimator.legodo.standing_schmitt_level=0.65|"
                       "state_estimator.legodo.torque_adjustment=true|state_estimator.legodo.adjustment_joints=l_leg_hpz,l_leg_kny,r_leg_kny|"
                       "state_estimator.legodo.adjustment_gain=7000,10000,10000");
  param.applyOverrides("state_estimator.scan_matcher.mode=position_yaw|state_estimator.scan_matcher.r_pxy=0.05|"
                       "state_estimator.scan_matcher.r_pz=0.05|state_estimator.scan_matcher.r_yaw=1.0");
  for (const char *sn : { "ins", "legodo", "scan_matcher" }) {
    param.set(std::string("state_estimator.") + sn + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + sn + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + sn + ".utime_offset", "0");
  }
}

// the logs `segs` as one batch (B = segs.size(); filter b starts from column segs[b] of the initial state)
// smooth: enableSmoothing + smooth(); else the two-argument EKFSmoothBackwardsPass
static Out run(const Setup &su, const std::vector<std::string> &paths, const std::vector<int> &segs, bool smooth, bool read = true)
{
  const int n = su.n, B = (int) segs.size();
  BotParam param;
  set_params(param, su);
  Out o;
  o.B = B;
  ModelClient model;
  if (!model.fromURDFString(URDF, "l_foot", "r_foot")) return o;
  RBIS x0(n, B);
  RBIM P0(n, B);
  for (int b = 0; b < B; b++) {
    const int s = segs[(size_t) b];
    for (int i = 0; i < n; i++) x0(i, b) = su.x0(i, s);
    for (int i = 0; i < 4; i++) x0.q(i, b) = su.x0.q(i, s);
    for (int c = 0; c < n; c++)
      for (int r = 0; r < n; r++) P0(r, c, b) = su.P0(r, c, s);
  }
  BotTrans ins_to_body;   // a mounted IMU: 90 degrees about z
  ins_to_body.rot_quat[0] = sqrt(0.5); ins_to_body.rot_quat[3] = sqrt(0.5);
  InsHandler ins_handler(&param, &ins_to_body);
  ScanMatcherHandler sm_handler(&param);
  FrontEnd front_end(&param);
  MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
  front_end.setStateEstimator(&est);
  LegOdoHandler legodo_handler(&param, &model);
  SegmentBatcher batch(&est);
  for (int b = 0; b < B; b++)
    if (!batch.addSegment(paths[(size_t) segs[(size_t) b]])) return o;
  batch.subscribeIns("IMU", su.schema, "bot_core.ins_t", front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler));
  batch.subscribeForceTorque("FORCE_TORQUE", su.schema, "bot_core.six_axis_force_torque_array_t",
                             [&](const msgs::six_axis_force_torque_array_t *m) { legodo_handler.forceTorqueHandler(m, B); });
  batch.subscribeJointState("JOINT_STATE", su.schema, "bot_core.joint_state_t", front_end.addSensor("legodo", &LegOdoHandler::processMessage, &legodo_handler));
  batch.subscribePose("POSE_SCAN", su.schema, "bot_core.pose_t", front_end.addSensor("scan_matcher", &ScanMatcherHandler::processMessage, &sm_handler));
  if (smooth && !batch.enableSmoothing()) return o;
  if (batch.run() < 0) return o;
  if (smooth) {
    RBIS h;
    RBIM c;
    batch.finalState(h, c);
    o.final_.vec = h.vec;
    o.final_.quat = h.quat;
    o.final_.cov = c.m;
  }
  est.flushPending();
  pb_sync(est.ctx);
  auto grab = [&](Call &c, int slot) {
    if (!read) return;
    c.vec.resize((size_t) n * B);
    c.quat.resize((size_t) 4 * B);
    c.cov.resize((size_t) n * n * B);
    if (pb_get_slot(est.ctx, slot, 0, B, c.vec.data(), c.quat.data(), c.cov.data(), nullptr, PB_HOST) != PB_OK) o.status = PB_ERR_STATE;
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (smooth) {
    o.ret = batch.smooth(SMOOTH_DT, [&](int step, int slot, const uint8_t *emit, const int64_t *utimes) {
      Call c;
      c.step = step;
      c.emit.assign(emit, emit + B);
      c.utimes.assign(utimes, utimes + B);
      grab(c, slot);
      o.calls.push_back(std::move(c));
    });
  } else {
    o.ret = est.EKFSmoothBackwardsPass(SMOOTH_DT, [&](int64_t utime, int slot) {
      Call c;
      c.utime = utime;
      grab(c, slot);
      o.calls.push_back(std::move(c));
    });
  }
  pb_sync(est.ctx);
  o.sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  o.status = o.status != PB_OK ? o.status : est.last_status;
  o.masked = est.smoother_masked_steps;
  o.fused = est.fused_pairs;
  o.reapplied = est.smoother_reapplied_updates;
  return o;
}

// block-relative difference of column b of call a against column c of call r (vec by max |vec|, quat absolute, cov by max |cov|)
static double col_err(int n, const Call &a, int Ba, int b, const Call &r, int Br, int c)
{
  double ev = 0, sv = 1e-300, eq = 0, eP = 0, sP = 1e-300;
  for (int i = 0; i < n; i++) {
    ev = fmax(ev, fabs(a.vec[(size_t) i * Ba + b] - r.vec[(size_t) i * Br + c]));
    sv = fmax(sv, fabs(r.vec[(size_t) i * Br + c]));
  }
  for (int i = 0; i < 4; i++) eq = fmax(eq, fabs(a.quat[(size_t) i * Ba + b] - r.quat[(size_t) i * Br + c]));
  for (int i = 0; i < n * n; i++) {
    eP = fmax(eP, fabs(a.cov[(size_t) i * Ba + b] - r.cov[(size_t) i * Br + c]));
    sP = fmax(sP, fabs(r.cov[(size_t) i * Br + c]));
  }
  return fmax(ev / sv, fmax(eq, eP / sP));
}

// (b) the oracle: segment s alone, forward (the filtered and predicted posterior of every tick), then the backward recursion
static double oracle_err(const Setup &su, const po_rbis &x_init, const po_rbim &P_init, const std::vector<Tick> &ticks, const std::vector<const Call *> &emitted,
                         int s, int Bbatch, const double q4[4], const ModelClient &model)
{
  const int n = su.n, Ts = (int) ticks.size();
  const char *adj[3] = { "l_leg_hpz", "l_leg_kny", "r_leg_kny" };
  const float gains[3] = { 7000.f, 10000.f, 10000.f };
  struct OChain { int n; int type[8], row[8]; double org[48], axis[24]; float gain[8]; } och[2];
  for (int side = 0; side < 2; side++) {
    const auto &ch = side ? model.right_chain : model.left_chain;
    och[side].n = (int) ch.size();
    for (int j = 0; j < och[side].n; j++) {
      och[side].type[j] = ch[(size_t) j].type;
      och[side].row[j] = (int) (std::find(JOINTS.begin(), JOINTS.end(), ch[(size_t) j].name) - JOINTS.begin());
      for (int i = 0; i < 3; i++) { och[side].org[6 * j + i] = ch[(size_t) j].xyz[i]; och[side].org[6 * j + 3 + i] = ch[(size_t) j].rpy[i]; och[side].axis[3 * j + i] = ch[(size_t) j].axis[i]; }
      och[side].gain[j] = 0.f;
      for (int a = 0; a < 3; a++) if (ch[(size_t) j].name == adj[a]) och[side].gain[j] = gains[a];
    }
  }
  BotTrans ins_to_body;
  ins_to_body.rot_quat[0] = sqrt(0.5); ins_to_body.rot_quat[3] = sqrt(0.5);
  const double r5[5] = { 2.0, 5.0, 3.0, 10.0, 9.0 };
  std::vector<char> leg(po_leg_sizeof());
  po_leg_init((po_leg *) leg.data(), 475, 525, 7000, 7000, 1);
  int zc = 3;
  po_rbis x = x_init;
  po_rbim P = P_init;
  double ll = 0;
  std::vector<po_rbis> pred_x((size_t) Ts), filt_x((size_t) Ts);
  std::vector<po_rbim> pred_P((size_t) Ts), filt_P((size_t) Ts);
  for (int k = 0; k < Ts; k++) {
    const Tick &tk = ticks[(size_t) k];
    double gb[3], ab[3];
    bot_quat_rotate_to(ins_to_body.rot_quat, tk.gyro, gb);
    bot_quat_rotate_to(ins_to_body.rot_quat, tk.accel, ab);
    po_imu_process_step(gb, ab, 0.002, q4[0], q4[1], q4[2], q4[3], &x, &P, ll, &x, &P, &ll);
    pred_x[(size_t) k] = x;
    pred_P[(size_t) k] = P;
    double ft_[2][3], fq_[2][4];
    for (int side = 0; side < 2; side++) {
      double ang[8];
      for (int j = 0; j < och[side].n; j++) {
        const int r = och[side].row[j];
        ang[j] = (double) po_torque_adjust(tk.jp[r], tk.je[r], och[side].gain[j]);
      }
      po_fk(och[side].n, och[side].type, och[side].org, och[side].axis, ang, ft_[side], fq_[side]);
    }
    double dt3[3], dq[4], cpos[3];
    long prev = 0;
    int cok = 0;
    const float status = po_leg_update_wc((po_leg *) leg.data(), tk.js_utime, ft_[0], fq_[0], ft_[1], fq_[1], fabs(tk.fz[0]), fabs(tk.fz[1]), -1, -1,
                                          &x.vec[9], x.quat, dt3, dq, &prev, cpos, &cok);
    if (status >= 0) {
      zc--;
      if (zc > 0) { dt3[0] = dt3[1] = dt3[2] = 0; dq[0] = 1; dq[1] = dq[2] = dq[3] = 0; }
      int idx[6];
      double z[6], Rd[6], R[36] = { 0 };
      const int m = po_legodo_create_measurement(0, r5, cpos, dt3, dq, tk.js_utime, prev, cok, status, idx, z, Rd);
      for (int i = 0; i < m; i++) R[i * m + i] = Rd[i];
      po_indexed_update(m, idx, z, R, &x, &P, ll, &x, &P, &ll);
    }
    if (tk.pose) {
      const int idx[4] = { 9, 10, 11, 8 };
      double z[4] = { tk.pos[0], tk.pos[1], tk.pos[2], 0.0 }, R[16] = { 0 };
      R[0] = R[5] = R[10] = 0.05 * 0.05;
      R[15] = bot_sq(bot_to_radians(1.0));
      po_indexed_orient_update(4, idx, z, R, tk.quat, &x, &P, ll, &x, &P, &ll);
    }
    filt_x[(size_t) k] = x;
    filt_P[(size_t) k] = P;
  }
  if ((int) emitted.size() != Ts - 1) return 1e300;
  po_rbis sx = filt_x[(size_t) Ts - 1];
  po_rbim sP = filt_P[(size_t) Ts - 1];
  double worst = 0;
  for (int k = Ts - 2; k >= 0; k--) {
    po_rbis cx = filt_x[(size_t) k];
    po_rbim cP = filt_P[(size_t) k];
    po_ekf_smoothing_step(&pred_x[(size_t) k + 1], &pred_P[(size_t) k + 1], &sx, &sP, SMOOTH_DT, &cx, &cP);
    sx = cx;
    sP = cP;
    const Call &c = *emitted[(size_t) (Ts - 2 - k)];
    if (c.step != k) return 1e300;
    Call o;   // the oracle's posterior as a one-column call
    o.vec.assign(sx.vec, sx.vec + n);
    o.quat.assign(sx.quat, sx.quat + 4);
    o.cov.resize((size_t) n * n);
    for (int cc = 0; cc < n; cc++)
      for (int rr = 0; rr < n; rr++) o.cov[(size_t) cc * n + rr] = sP.m[cc * 21 + rr];
    worst = fmax(worst, col_err(n, c, Bbatch, s, o, 1, 0));
  }
  return worst;
}

int main(int argc, char **argv)
{
  const int n = take_n_states(argc, argv);
  bool fuse = true, timing = false;
  int every = 1;
  std::string dir = "/tmp";
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "nofuse") fuse = false;
    else if (a == "time") timing = true;
    else if (a.rfind("every=", 0) == 0) every = atoi(a.c_str() + 6);
    else if (a[0] == '/') dir = a;
  }
  double g;
  po_get_constants(&g, nullptr);
  pronto_wire::Schema schema;
  std::string err;
  if (!schema.parse(BOT_CORE_LCM, &err)) { printf("schema: %s\nFAIL\n", err.c_str()); return 1; }
  std::vector<std::vector<Tick>> ticks, ticks_eq;
  std::vector<std::string> paths, paths_eq;
  if (!write_logs(dir, "ragged", true, g, schema, ticks, paths) || !write_logs(dir, "equal", false, g, schema, ticks_eq, paths_eq)) {
    printf("cannot write the logs\nFAIL\n");
    return 1;
  }
  // initial states: another heading per log (and a bias prior for 21 states)
  Setup su{ n, fuse, every, &schema, RBIS(n, NSEG), RBIM(n, NSEG) };
  std::vector<po_rbis> ox(NSEG);
  std::vector<po_rbim> oP(NSEG);
  rng_state = 0x1234567ULL;
  for (int b = 0; b < NSEG; b++) {
    double q[4];
    po_euler_to_quat(0.05 * (urand() - 0.5), 0.05 * (urand() - 0.5), 6.0 * (urand() - 0.5), q);
    po_rbis_zero(&ox[(size_t) b]);
    memset(&oP[(size_t) b], 0, sizeof(po_rbim));
    for (int i = 0; i < 4; i++) { su.x0.q(i, b) = q[i]; ox[(size_t) b].quat[i] = q[i]; }
    const double sig[15] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0 };
    for (int i = 0; i < 15; i++) { su.P0(i, i, b) = sig[i] * sig[i]; oP[(size_t) b].m[i * 21 + i] = sig[i] * sig[i]; }
    init_bias_states(n, b, su.x0, su.P0, &ox[(size_t) b], &oP[(size_t) b], urand);
  }
  std::vector<int> all(NSEG);
  for (int s = 0; s < NSEG; s++) all[(size_t) s] = s;

  // ---- (a) the ragged batch against 64 single-segment runs ----
  const Out bat = run(su, paths, all, true);
  bool ok = bat.ret == (int) bat.calls.size() && bat.status == PB_OK && bat.masked > 0 && (!fuse || bat.fused > 0);
  if (!ok) printf("ragged batch: smooth() returned %d for %zu sink calls, status %d, masked steps %lld, fused pairs %lld\n", bat.ret, bat.calls.size(),
                  bat.status, (long long) bat.masked, (long long) bat.fused);
  double err_a = 0;
  int count_bad = 0;
  std::vector<std::vector<const Call *>> per_seg(NSEG);
  for (const Call &c : bat.calls)
    for (int s = 0; s < NSEG; s++)
      if (c.emit[(size_t) s]) per_seg[(size_t) s].push_back(&c);
  for (int s = 0; s < NSEG; s++) {
    const Out one = run(su, paths, { s }, false);
    const int Ts = (int) ticks[(size_t) s].size();
    if (one.status != PB_OK || one.ret != Ts - 1 || (int) per_seg[(size_t) s].size() != Ts - 1 || (int) one.calls.size() != Ts - 1) {
      if (count_bad++ < 4)
        printf("segment %d: %zu emitted, single run returned %d with %zu calls (status %d), %d INS updates\n", s, per_seg[(size_t) s].size(), one.ret,
               one.calls.size(), one.status, Ts);
      ok = false;
      continue;
    }
    for (int c = 0; c < Ts - 1; c++) {
      const Call &bc = *per_seg[(size_t) s][(size_t) c];
      if (bc.step != Ts - 2 - c || bc.utimes[(size_t) s] != one.calls[(size_t) c].utime || bc.utimes[(size_t) s] != ticks[(size_t) s][(size_t) bc.step].imu_utime) {
        if (count_bad++ < 4)
          printf("segment %d, emit %d: step %d (want %d), utime %" PRId64 " / single run %" PRId64 " / log %" PRId64 "\n", s, c, bc.step, Ts - 2 - c,
                 bc.utimes[(size_t) s], one.calls[(size_t) c].utime, ticks[(size_t) s][(size_t) (Ts - 2 - c)].imu_utime);
        ok = false;
      }
      err_a = fmax(err_a, col_err(n, bc, NSEG, s, one.calls[(size_t) c], 1, 0));
    }
  }

  // ---- (b) four segments against the oracle directly ----
  double err_b = 0;
  {
    ModelClient model;
    model.fromURDFString(URDF, "l_foot", "r_foot");
    BotParam p;
    set_params(p, su);
    BotTrans itb;
    InsHandler ih(&p, &itb);
    const double q4[4] = { ih.cov_gyro, ih.cov_accel, ih.cov_gyro_bias, ih.cov_accel_bias };
    for (int s : { 0, 1, 7, 8 })
      err_b = fmax(err_b, oracle_err(su, ox[(size_t) s], oP[(size_t) s], ticks[(size_t) s], per_seg[(size_t) s], s, NSEG, q4, model));
  }

  // ---- (c) equal lengths: smooth() is the two-argument pass, bit for bit, without a select launch ----
  const Out eq_new = run(su, paths_eq, all, true), eq_old = run(su, paths_eq, all, false);
  bool same_c = eq_new.status == PB_OK && eq_old.status == PB_OK && eq_new.ret > 0 && eq_new.ret == eq_old.ret && eq_new.calls.size() == eq_old.calls.size() &&
                eq_new.masked == 0;
  for (size_t c = 0; same_c && c < eq_new.calls.size(); c++) {
    const Call &a = eq_new.calls[c], &b = eq_old.calls[c];
    same_c = a.vec.size() == b.vec.size() && a.cov.size() == b.cov.size() && memcmp(a.vec.data(), b.vec.data(), sizeof(double) * a.vec.size()) == 0 &&
             memcmp(a.quat.data(), b.quat.data(), sizeof(double) * a.quat.size()) == 0 && memcmp(a.cov.data(), b.cov.data(), sizeof(double) * a.cov.size()) == 0;
    for (int s = 0; same_c && s < NSEG; s++) same_c = a.emit[(size_t) s] == 1;   // (every segment has a later INS update at every smoothed tick)
  }

  // ---- (d) after a segment's end its rows carry its final posterior (the terminal slot), bit for bit.  The two-argument pass on the
  // ---- same batch does not: there its rows after the end hold the idle state, not bit for bit the final posterior (asserted per segment
  // ---- that ends early).  Its EMITTED rows are printed only: they agree to rounding here (an idle tick's predicted and carried states
  // ---- are one and the same idle state).
  const Out old = run(su, paths, all, false);
  bool d_ok = old.status == PB_OK && old.calls.size() == bat.calls.size() && old.ret == bat.ret;
  double old_emit = 0, old_idle = 1e300;
  int idle_rows = 0;
  for (int s = 0; d_ok && s < NSEG; s++) {
    const int Ts = (int) ticks[(size_t) s].size();
    double old_idle_s = 0;
    for (size_t c = 0; c < bat.calls.size(); c++) {
      const Call &bc = bat.calls[c];
      if (bc.emit[(size_t) s]) old_emit = fmax(old_emit, col_err(n, old.calls[c], NSEG, s, bc, NSEG, s));
      if (bc.step < Ts - 1) continue;
      idle_rows++;   // a tick at or after this segment's last INS update: the row is its final posterior, carried
      for (int i = 0; i < n; i++) d_ok = d_ok && memcmp(&bc.vec[(size_t) i * NSEG + s], &bat.final_.vec[(size_t) i * NSEG + s], 8) == 0;
      for (int i = 0; i < 4; i++) d_ok = d_ok && memcmp(&bc.quat[(size_t) i * NSEG + s], &bat.final_.quat[(size_t) i * NSEG + s], 8) == 0;
      for (int i = 0; i < n * n; i++) d_ok = d_ok && memcmp(&bc.cov[(size_t) i * NSEG + s], &bat.final_.cov[(size_t) i * NSEG + s], 8) == 0;
      if (bc.step >= Ts) old_idle_s = fmax(old_idle_s, col_err(n, old.calls[c], NSEG, s, bat.final_, NSEG, s));
    }
    if (Ts < T_MAX) old_idle = fmin(old_idle, old_idle_s);
  }
  const bool carry_ok = d_ok && idle_rows > 0, old_differs = old_idle > 0;
  d_ok = carry_ok && old_differs;

  printf("n=%d %s every=%d: 64 segments of %d..%d ticks, %zu smoothed ticks, %lld select launches, fused pairs %lld, re-applied updates %lld\n"
         "  (a) vs 64 single-segment passes: rel err %.2e%s\n  (b) segments 0 1 7 8 vs the oracle's recursion: rel err %.2e\n"
         "  (c) equal lengths, smooth() vs the two-argument pass: %s (%d steps, %lld select launches)\n"
         "  (d) %d rows after a segment's end: %s its final posterior; the two-argument pass: %s there (relative difference of at least %.2e "
         "for every early-ending segment), %.2e from (a) on the emitted rows\n",
         n, fuse ? "fused" : "unfused", every, T_MAX - 8 * 8, T_MAX, bat.calls.size(), (long long) bat.masked, (long long) bat.fused,
         (long long) bat.reapplied, err_a, count_bad ? " (count / order mismatches)" : "", err_b, same_c ? "bit-identical" : "DIFFERENT", eq_new.ret,
         (long long) eq_new.masked, idle_rows, carry_ok ? "bit for bit" : "NOT", old_differs ? "not it" : "THE SAME", old_idle, old_emit);
  ok = ok && count_bad == 0 && err_a < 1e-9 && err_b < 1e-9 && same_c && d_ok;

  if (timing) {   // wall time of the backward pass alone (nothing read back): one ragged batch against 64 single-segment passes
    const Out tb = run(su, paths, all, true, false);
    double single = 0;
    for (int s = 0; s < NSEG; s++) single += run(su, paths, { s }, false, false).sec;
    printf("  smooth() of the 64-segment batch %.1f ms, 64 single-segment passes %.1f ms in all (%.1fx)\n", tb.sec * 1e3, single * 1e3, single / tb.sec);
  }
  printf(ok ? "PASS\n" : "FAIL\n");
  for (int s = 0; s < NSEG; s++) {
    remove(paths[(size_t) s].c_str());
    remove(paths_eq[(size_t) s].c_str());
  }
  return ok ? 0 : 1;
}
