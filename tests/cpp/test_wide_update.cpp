// test_wide_update.cpp -- a recorded log whose GPF_MEASUREMENT messages carry the all_states list {3..11} (velocity, chi, position;
// rgbd_gpf_lib.cpp:86-91) with a full R, between IMU messages, replayed through LogPlayer + WideIndexedMeasurementHandler
// (pronto_amd/csrc/mav_state_est_wide.hpp) into 70 filters with posterior checkpoints on, against the oracle filter by filter.  Then the
// same messages with one GPF message delivered three IMU steps late: the history restores a checkpoint and re-applies the nine-row update
// with what follows, and the head must equal the in-order oracle to the same bound.  Exit code 0 + "PASS".  Needs a GPU.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "test_n.hpp"
#include "../../pronto_amd/csrc/mav_state_est_wide.hpp"

using namespace MavStateEst;

static uint64_t rng_state = 0x574944455550ULL;
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
  const std::string logs[2] = { dir + "/wide_inorder.lcmlog", dir + "/wide_late.lcmlog" };
  const int B = 70, T = 40, LATE_K = 19, DELAY = 3;
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

  // ---- record the messages once, write them in order and with message LATE_K's GPF event DELAY steps behind its time ----
  {
    std::vector<std::vector<uint8_t>> imu(T), gpf(T);
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
      if (k % 5 == 4) {
        pronto_wire::indexed_measurement_t im;
        im.utime = utime;
        im.state_utime = utime - 1000;
        im.measured_dim = 9;
        im.measured_cov_dim = 81;
        im.R_effective.assign(81, 0.0);
        for (int i = 0; i < 9; i++) {
          im.z_indices.push_back(3 + i);
          im.z_effective.push_back((i >= 3 && i < 6 ? 0.02 : 0.2) * nrand());
          for (int j = 0; j <= i; j++) {
            const double r = i == j ? (i >= 3 && i < 6 ? 0.002 : 0.02) * (1.0 + 0.1 * i) : 0.0005 * (urand() - 0.5);
            im.R_effective[(size_t) j * 9 + i] = im.R_effective[(size_t) i * 9 + j] = r;
          }
        }
        im.encode(gpf[k]);
      }
    }
    for (int late = 0; late < 2; late++) {
      pronto_wire::LogWriter log(logs[late]);
      if (!log.good()) { printf("cannot write %s\nFAIL\n", logs[late].c_str()); return 1; }
      for (int k = 0; k < T; k++) {
        const int64_t utime = (int64_t) (k + 1) * 1000;
        log.write(utime, "IMU_TICK", imu[k]);
        if (!gpf[k].empty() && !(late && k == LATE_K)) log.write(utime, "GPF_MEASUREMENT", gpf[k]);
        if (late && k == LATE_K + DELAY) log.write(utime, "GPF_MEASUREMENT", gpf[LATE_K]);
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
  for (const char *s : { "ins", "gpf" }) {
    param.set(std::string("state_estimator.") + s + ".downsample_factor", "1");
    param.set(std::string("state_estimator.") + s + ".roll_forward_on_receive", "true");
    param.set(std::string("state_estimator.") + s + ".utime_offset", "0");
  }
  RBIS x0(n, B);
  RBIM P0(n, B);
  std::vector<po_rbis> ox(B);
  std::vector<po_rbim> oP(B);
  std::vector<double> oll(B, 0.0);
  for (int b = 0; b < B; b++) {
    double q[4];
    po_euler_to_quat(0.1 * (urand() - 0.5), 0.1 * (urand() - 0.5), 6.0 * (urand() - 0.5), q);
    po_rbis_zero(&ox[b]);
    memset(&oP[b], 0, sizeof(po_rbim));
    for (int i = 0; i < 4; i++) { x0.q(i, b) = q[i]; ox[b].quat[i] = q[i]; }
    for (int i = 0; i < 3; i++) { x0(3 + i, b) = 0.2 * nrand(); ox[b].vec[3 + i] = x0(3 + i, b); }
    const double sig[15] = { 0, 0, 0, .15, .15, .15, .05, .05, .05, .5, .5, .5, 0, 0, 0 };
    for (int i = 0; i < 15; i++) { P0(i, i, b) = sig[i] * sig[i] * (1.0 + 0.01 * b); oP[b].m[i * 21 + i] = P0(i, i, b); }
    init_bias_states(n, b, x0, P0, &ox[b], &oP[b], urand);
  }
  BotTrans ins_to_body;
  bool ok = true;
  for (int late = 0; late < 2; late++) {
    InsHandler ins_handler(&param, &ins_to_body);
    WideIndexedMeasurementHandler gpf_handler(RBISUpdateInterface::laser_gpf);
    FrontEnd front_end(&param);
    auto on_ins = front_end.addSensor("ins", &InsHandler::processMessage, &ins_handler);
    auto on_gpf = front_end.addSensor("gpf", &WideIndexedMeasurementHandler::processMessage, &gpf_handler);
    MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
    front_end.setStateEstimator(&est);
    const double q4[4] = { ins_handler.cov_gyro, ins_handler.cov_accel, ins_handler.cov_gyro_bias, ins_handler.cov_accel_bias };
    LogPlayer player(B);
    int n_imu = 0, n_gpf = 0;
    // (the oracle runs the in-order log only: the late delivery must end where that one ends)
    player.subscribeIns("IMU_TICK", &ins_schema, "test_core.ins_t", [&](const msgs::ins_t *m) {
      const double v[6] = { m->gyro.p[0], m->gyro.p[1], m->gyro.p[2], m->accel.p[0], m->accel.p[1], m->accel.p[2] };
      on_ins(m);
      for (int b = 0; b < B && !late; b++)
        po_imu_process_step(v, v + 3, 0.001, q4[0], q4[1], q4[2], q4[3], &ox[b], &oP[b], oll[b], &ox[b], &oP[b], &oll[b]);
      n_imu++;
    });
    player.subscribeIndexedMeasurement("GPF_MEASUREMENT", [&](const msgs::indexed_measurement_t *m) {
      on_gpf(m);
      for (int b = 0; b < B && !late; b++)
        po_indexed_update((int) m->z_indices.size(), m->z_indices.data(), m->z_effective.p, m->R_effective, &ox[b], &oP[b], oll[b], &ox[b], &oP[b], &oll[b]);
      n_gpf++;
    });
    const int64_t dispatched = player.run(logs[late]);
    RBIS head;
    RBIM cov;
    est.getHeadState(head, cov);
    std::vector<double> ll = est.getMeasurementsLogLikelihood();
    double ev = 0, eq = 0, eP = 0, el = 0, sv = 0, sP = 0, sl = 0;
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < n; i++) { ev = fmax(ev, fabs(head(i, b) - ox[b].vec[i])); sv = fmax(sv, fabs(ox[b].vec[i])); }
      for (int i = 0; i < 4; i++) eq = fmax(eq, fabs(head.q(i, b) - ox[b].quat[i]));
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) { eP = fmax(eP, fabs(cov(r, c, b) - oP[b].m[c * 21 + r])); sP = fmax(sP, fabs(oP[b].m[c * 21 + r])); }
      el = fmax(el, fabs(ll[b] - oll[b]));
      sl = fmax(sl, fabs(oll[b]));
    }
    printf("%s: %" PRId64 " events (imu %d, gpf %d, undecodable %" PRId64 ", replayed %jd): rel err vec %.2e quat %.2e cov %.2e ll %.2e (status %d)\n",
           late ? "one message late" : "in order", dispatched, n_imu, n_gpf, player.undecodable(), (intmax_t) est.replayed_updates, ev / sv, eq, eP / sP,
           el / sl, est.last_status);
    ok = ok && est.last_status == PB_OK && dispatched == n_imu + n_gpf && n_imu == T && n_gpf == T / 5 && player.undecodable() == 0 &&
         est.dropped_updates == 0 && est.replayed_updates == (late ? DELAY : 0) /* the IMU steps behind the late update; itself it is applied, not replayed */ && head.utime == (int64_t) T * 1000 &&
         ev / sv < 1e-9 && eq < 1e-9 && eP / sP < 1e-9 && el / sl < 1e-9;
  }
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
