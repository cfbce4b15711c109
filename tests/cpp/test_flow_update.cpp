// test_flow_update.cpp -- a short written log of IMU messages with two pronto::optical_flow_t messages (one robot's message for every
// filter) replayed through LogPlayer + OpticalFlowHandler (pronto_amd/csrc/mav_state_est_flow.hpp) into 70 filters with posterior
// checkpoints on.  Then the same messages with the first flow message delivered three IMU steps late: the history restores a checkpoint
// and re-applies the update, which owns its message and draws nothing, so the two heads must be EQUAL, value for value.  Also: the
// updates moved the velocity (against a run without flow messages), and every value is finite.
// Exit code 0 + "PASS".  Needs a GPU.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "test_n.hpp"
#include "../../pronto_amd/csrc/mav_state_est_flow.hpp"

using namespace MavStateEst;

static uint64_t rng_state = 0x464c4f57ULL;
static double urand()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }

int main(int argc, char **argv)
{
  const int n = take_n_states(argc, argv);
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string logs[3] = { dir + "/flow_inorder.lcmlog", dir + "/flow_late.lcmlog", dir + "/flow_none.lcmlog" };
  const int B = 70, T = 30, FLOW_A = 9, FLOW_B = 19, DELAY = 3;
  double g;
  po_get_constants(&g, nullptr);

  pronto_wire::Schema ins_schema;
  {
    std::string err;
    const bool parsed = ins_schema.parse(
        "package test_core;\n"
        "struct ins_t {\n"
        "  int64_t utime;  int64_t device_time;\n"
        "  double gyro[3];  double mag[3];  double accel[3];  double quat[4];\n"
        "  double pressure;  double rel_alt;\n"
        "}\n", &err);
    if (!parsed || ins_schema.fingerprint("ins_t") == 0) { printf("schema: %s\nFAIL\n", err.c_str()); return 1; }
  }

  // ---- the messages, written in order, with flow A's event DELAY steps behind its time, and without flow messages ----
  {
    std::vector<std::vector<uint8_t>> imu(T), flow(T);
    for (int k = 0; k < T; k++) {
      const int64_t utime = (int64_t) (k + 1) * 1000;
      pronto_wire::Writer w;
      w.u64(ins_schema.fingerprint("test_core.ins_t"));
      w.i64(utime);
      w.i64(utime + 17);
      for (int i = 0; i < 3; i++) w.f64(0.3 * sin(0.02 * k + i) + 0.01 * nrand());
      for (int i = 0; i < 3; i++) w.f64(0.1 * i);
      for (int i = 0; i < 3; i++) w.f64(0.3 * nrand() + (i == 2 ? g : 0.0));
      for (int i = 0; i < 4; i++) w.f64(i == 0);
      w.f64(1013.0);
      w.f64(0.0);
      imu[k] = w.buf;
      if (k == FLOW_A || k == FLOW_B) {
        pronto_wire::optical_flow_t m;
        m.utime = utime;
        m.dt = 0.03;
        m.ux = 0.05 + 0.02 * nrand();
        m.uy = -0.08 + 0.02 * nrand();
        m.theta = 0.01 * nrand();
        m.scale = 0.02 * nrand();
        m.alpha1 = 1.02;
        m.alpha2 = 0.97;
        m.gamma = 1.05;
        m.encode(flow[k]);
      }
    }
    for (int v = 0; v < 3; v++) {
      pronto_wire::LogWriter log(logs[v]);
      if (!log.good()) { printf("cannot write %s\nFAIL\n", logs[v].c_str()); return 1; }
      for (int k = 0; k < T; k++) {
        const int64_t utime = (int64_t) (k + 1) * 1000;
        log.write(utime, "IMU_TICK", imu[k]);
        if (v == 2) continue;
        if (!flow[k].empty() && !(v == 1 && k == FLOW_A)) log.write(utime, "OPTICAL_FLOW", flow[k]);
        if (v == 1 && k == FLOW_A + DELAY) log.write(utime, "OPTICAL_FLOW", flow[FLOW_A]);
      }
    }
  }

  BotParam param;
  param.set("state_estimator.utime_history_span", "1000000");
  param.set("state_estimator.history_slots", "64");
  param.set("state_estimator.ins.channel", "IMU_TICK");
  param.set("state_estimator.ins.q_gyro", 0.5);
  param.set("state_estimator.ins.q_accel", 0.1);
  param.set("state_estimator.ins.timestep_dt", 0.001);
  param.set("state_estimator.ins.atlas_filter", "false");
  set_ins_bias_keys(param, n);
  for (const char *s : { "ins", "optical_flow" }) {
    param.set(std::string("state_estimator.") + s + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + s + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + s + ".utime_offset", "0");
  }
  param.set("state_estimator.optical_flow.r_ux", 0.05);
  param.set("state_estimator.optical_flow.r_uy", 0.05);
  param.set("state_estimator.optical_flow.r_r", 0.02);
  param.set("state_estimator.optical_flow.r_s", 0.02);

  // a camera looking down, tilted 0.1 rad about x, 0.1 m in front of the body origin
  BotTrans body_to_cam;
  body_to_cam.rot_quat[0] = cos(0.5 * (M_PI + 0.1));
  body_to_cam.rot_quat[1] = sin(0.5 * (M_PI + 0.1));
  body_to_cam.trans_vec[0] = 0.1; body_to_cam.trans_vec[1] = 0.02; body_to_cam.trans_vec[2] = -0.05;

  RBIS x0(n, B);
  RBIM P0(n, B);
  std::vector<po_rbis> ox(B);
  std::vector<po_rbim> oP(B);
  for (int b = 0; b < B; b++) {
    double q[4];
    po_euler_to_quat(0.1 * (urand() - 0.5), 0.1 * (urand() - 0.5), 6.0 * (urand() - 0.5), q);
    po_rbis_zero(&ox[b]);
    memset(&oP[b], 0, sizeof(po_rbim));
    for (int i = 0; i < 4; i++) x0.q(i, b) = q[i];
    for (int i = 0; i < 3; i++) x0(3 + i, b) = 0.2 * nrand();
    for (int i = 0; i < 2; i++) x0(9 + i, b) = 0.3 * nrand();
    x0(11, b) = 1.0 + 3.0 * urand();  // the height over the ground
    const double sig[15] = { .02, .02, .02, .15, .15, .15, .05, .05, .05, .5, .5, .3, 0, 0, 0 };
    for (int i = 0; i < 15; i++) P0(i, i, b) = sig[i] * sig[i] * (1.0 + 0.01 * b);
    init_bias_states(n, b, x0, P0, &ox[b], &oP[b], urand);
  }
  BotTrans ins_to_body;
  bool ok = true;
  RBIS heads[3];
  RBIM covs[3];
  std::vector<double> lls[3];
  for (int v = 0; v < 3; v++) {
    InsHandler ins_handler(&param, &ins_to_body);
    OpticalFlowHandler flow_handler(&param, &body_to_cam);
    FrontEnd front_end(&param);
    auto on_ins = front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler);
    auto on_flow = front_end.addSensor("optical_flow", &OpticalFlowHandler::processMessage, &flow_handler);
    MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
    front_end.setStateEstimator(&est);
    LogPlayer player(B);
    int n_imu = 0, n_flow = 0;
    player.subscribeIns("IMU_TICK", &ins_schema, "test_core.ins_t", [&](const msgs::ins_t *m) {
      on_ins(m);
      n_imu++;
    });
    player.subscribeRaw("OPTICAL_FLOW", [&](const pronto_wire::LogEvent &ev) {
      pronto_wire::optical_flow_t wire;
      if (wire.decode(ev.data.data(), ev.data.size()) < 0) return;
      msgs::optical_flow_t msg;
      msg.utime = wire.utime;
      msg.set(wire.ux, wire.uy, wire.theta, wire.scale, wire.alpha1, wire.alpha2, wire.gamma);
      on_flow(&msg);
      n_flow++;
    });
    const int64_t dispatched = player.run(logs[v]);
    est.getHeadState(heads[v], covs[v]);
    lls[v] = est.getMeasurementsLogLikelihood();
    printf("%s: %" PRId64 " events (imu %d, flow %d, replayed %jd, dropped %jd, status %d)\n",
           v == 0 ? "in order" : (v == 1 ? "first flow message late" : "no flow messages"), dispatched, n_imu, n_flow, (intmax_t) est.replayed_updates,
           (intmax_t) est.dropped_updates, est.last_status);
    ok = ok && est.last_status == PB_OK && dispatched == n_imu + n_flow && n_imu == T && n_flow == (v == 2 ? 0 : 2) && est.dropped_updates == 0 &&
         est.replayed_updates == (v == 1 ? DELAY : 0) && heads[v].utime == (int64_t) T * 1000;
  }
  // in order against late: equal; in order against no flow messages: the velocity moved; everything finite
  size_t diff = 0, nonfinite = 0;
  double moved = 0.0;
  for (size_t i = 0; i < heads[0].vec.size(); i++) {
    diff += heads[0].vec[i] != heads[1].vec[i];
    nonfinite += !std::isfinite(heads[0].vec[i]);
  }
  for (size_t i = 0; i < heads[0].quat.size(); i++) diff += heads[0].quat[i] != heads[1].quat[i];
  for (size_t i = 0; i < covs[0].m.size(); i++) {
    diff += covs[0].m[i] != covs[1].m[i];
    nonfinite += !std::isfinite(covs[0].m[i]);
  }
  for (int b = 0; b < B; b++) {
    diff += lls[0][b] != lls[1][b];
    for (int i = 3; i < 6; i++) moved = fmax(moved, fabs(heads[0](i, b) - heads[2](i, b)));
  }
  printf("in order against first flow message late: %zu values differ; non-finite %zu; largest velocity change by the flow messages %.3e\n", diff,
         nonfinite, moved);
  ok = ok && diff == 0 && nonfinite == 0 && moved > 1e-3;
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
