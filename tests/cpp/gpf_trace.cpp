// gpf_trace.cpp -- what LaserGPFHandler, GridLikelihood and RBISGPFMeasurement (pronto_amd/csrc/mav_state_est_gpf.hpp) ask the device to do,
// recorded on the CPU against tests/cpp/abi_recorder.cpp + abi_recorder_wide.cpp + abi_recorder_gpf.cpp (no HIP, no library).  Each
// scenario prints every pb_* call, the handler's and the estimator's own messages and what the handler returned; tests/test_gpf_trace.py
// compares with tests/golden/gpf_trace/<scenario>.txt.
//   pos_only, pos_yaw, pos_chi, all_states, z_only   one broadcast scan through each substate list
//   per_filter_scan   a scan with points per filter (PB_HOST): the likelihood owns a copy
//   late_scan         history_checkpoint_every = 1; a scan arrives late, then a position fix in front of both scans: the history
//                     re-applies each GPF update, which asks for the SAME stream_id as the first time
//   bad_substate      the reference's fatal error (exit code 1)
//   zero_samples      gpf_num_samples = 0: no call, NULL
#include <cinttypes>
#include <cstdio>
#include <deque>
#include <memory>
#include <unistd.h>

#ifndef SHIM_HEADER
#define SHIM_HEADER "../../pronto_amd/csrc/mav_state_est_gpf.hpp"
#endif
#include SHIM_HEADER
#include "abi_recorder.h"

using namespace MavStateEst;
typedef RBISUpdateInterface U;

static std::vector<double> vals(size_t k, double seed)
{
  std::vector<double> v(k);
  for (size_t i = 0; i < k; i++) v[i] = seed + 0.001 * (double) i;
  return v;
}

struct Sc {
  int B = 2, n = 15;
  BotParam param;
  std::unique_ptr<MavStateEstimator> est;
  std::unique_ptr<LaserGPFHandler> handler;
  std::deque<std::vector<double>> arena;
  const double q[4] = { 7.6e-5, 0.01, 3e-10, 1e-8 };

  Sc(const char *substate, const char *samples, std::initializer_list<std::pair<const char *, const char *>> kv)
  {
    param.set("state_estimator.utime_history_span", 1000000.0);
    param.set("state_estimator.laser_gpf.gpf_num_samples", samples);
    param.set("state_estimator.laser_gpf.gpf_substate", substate);
    param.set("state_estimator.laser_gpf.max_weight_proportion", 0.999);
    param.set("state_estimator.laser_gpf.unknown_loglike", -12.0);
    param.set("state_estimator.laser_gpf.sigma_scaling", 1.5);
    param.set("state_estimator.laser_gpf.seed", "42");
    for (auto &p : kv) param.set(p.first, p.second);
    auto map = std::make_shared<GridMap>();
    map->origin[0] = -3.0; map->origin[1] = -2.5; map->origin[2] = -1.0;
    map->resolution = 0.5;
    map->dims[0] = 4; map->dims[1] = 3; map->dims[2] = 2;
    map->values = vals(24, -2.0);
    handler.reset(new LaserGPFHandler(&param, map));
    RBIS x0(n, B);
    RBIM P0(n, B);
    x0.vec = vals(x0.vec.size(), 0.5);
    P0.m = vals(P0.m.size(), 0.25);
    est.reset(new MavStateEstimator(new RBISResetUpdate(x0, P0, U::reset, 0), &param, 0));
  }
  ~Sc()
  {
    const MavStateEstimator &e = *est;
    printf("= replayed %jd dropped %jd status %d head_utime %jd history %zu\n", (intmax_t) e.replayed_updates, (intmax_t) e.dropped_updates,
           e.last_status, (intmax_t) e.head_utime, e.history.updateMap.size());
    handler.reset();
    est.reset();
  }
  double *keep(size_t k, double seed) { arena.push_back(vals(k, seed)); return arena.back().data(); }
  // a scan of n_points at time t; form 'b' one robot's points for every filter, 'h' points per filter
  U *scan(int64_t t, int n_points, char form)
  {
    msgs::scan_points_t msg;
    msg.utime = t;
    msg.n_points = n_points;
    msg.points = form == 'b' ? BatchArray(keep((size_t) 3 * n_points, 1e-6 * t), PB_HOST_BROADCAST)
                             : BatchArray(keep((size_t) 3 * n_points * B, 1e-6 * t), PB_HOST);
    U *u = handler->processMessage(&msg, est.get());
    if (u == nullptr) {
      printf("# processMessage t=%jd -> NULL\n", (intmax_t) t);
      return nullptr;
    }
    auto *g = dynamic_cast<RBISGPFMeasurement *>(u);
    auto *lk = dynamic_cast<GridLikelihood *>(g->likelihood.get());
    printf("# processMessage t=%jd -> RBISGPFMeasurement sensor=%s m=%zu K=%d stream_id=%u seed=%ju owns_points=%zu points_mem=%d\n", (intmax_t) t,
           U::sensor_enum_string(u->sensor_id), g->index.size(), g->K, g->stream_id, (uintmax_t) g->seed, lk->owned_points.size(), lk->points_mem);
    return u;
  }
  void add(U *u)
  {
    if (u == nullptr) return;
    printf("# add %s t=%jd\n", U::sensor_enum_string(u->sensor_id), (intmax_t) u->utime);
    est->addUpdate(u, true);
  }
  void imu(int64_t t) { add(new RBISIMUProcessStep(vals(7, 1e-6 * t), q[0], q[1], q[2], q[3], t, PB_HOST_BROADCAST)); }
};

#define SLOTS(s) { "state_estimator.history_slots", s }
#define EVERY(s) { "state_estimator.history_checkpoint_every", s }

static void one_scan(const char *substate)
{
  Sc s(substate, "16", { SLOTS("0") });
  s.imu(1000);
  s.add(s.scan(1000, 5, 'b'));
  s.imu(2000);
  s.add(s.scan(2000, 4, 'b'));
}
static void pos_only() { one_scan("pos_only"); }
static void pos_yaw() { one_scan("pos_yaw"); }
static void pos_chi() { one_scan("pos_chi"); }
static void all_states() { one_scan("all_states"); }
static void z_only() { one_scan("z_only"); }
static void per_filter_scan()
{
  Sc s("pos_chi", "8", { SLOTS("0") });
  s.imu(1000);
  s.add(s.scan(1000, 3, 'h'));
}
static void late_scan()
{
  Sc s("pos_yaw", "8", { SLOTS("8"), EVERY("1") });
  s.imu(1000);
  s.imu(2000);
  s.imu(3000);
  s.add(s.scan(1500, 5, 'b'));   // late: restore the checkpoint in front of it, then it and the two steps behind it
  s.imu(4000);
  s.add(s.scan(2500, 4, 'b'));   // late again: the first scan's update stays where it is
  // a position fix in front of both: both GPF updates are re-applied, each with the stream_id it was made with
  s.add(new RBISIndexedMeasurement(RBIS::positionInds(), vals((size_t) 3 * s.B, 0.0036), vals(3, 4e-4), PB_R_DIAG_BROADCAST, {}, U::gps, 1200));
}
static void bad_substate() { one_scan("pos_and_velocity"); }
static void zero_samples()
{
  Sc s("pos_only", "0", { SLOTS("0") });
  s.imu(1000);
  s.add(s.scan(1000, 5, 'b'));
}

static const struct {
  const char *name;
  void (*run)();
} SCENARIOS[] = { { "pos_only", pos_only },   { "pos_yaw", pos_yaw },     { "pos_chi", pos_chi },           { "all_states", all_states },    { "z_only", z_only },
                  { "per_filter_scan", per_filter_scan }, { "late_scan", late_scan }, { "bad_substate", bad_substate }, { "zero_samples", zero_samples } };

int main(int argc, char **argv)
{
  // one unbuffered stream: the handler's and the estimator's stderr messages land between the calls that surround them
  dup2(STDOUT_FILENO, STDERR_FILENO);
  setvbuf(stdout, nullptr, _IONBF, 0);
  setvbuf(stderr, nullptr, _IONBF, 0);
  for (const auto &sc : SCENARIOS) {
    if (argc == 2 && std::string(argv[1]) == "--list") printf("%s\n", sc.name);
    else if (argc == 2 && std::string(argv[1]) == sc.name) {
      sc.run();
      return 0;
    }
  }
  if (argc == 2 && std::string(argv[1]) == "--list") return 0;
  fprintf(stderr, "usage: gpf_trace --list | <scenario>\n");
  return 2;
}
