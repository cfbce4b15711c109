// estimator_trace.cpp -- MavStateEstimator and the update objects (pronto_amd/csrc/mav_state_est.hpp) driven on the CPU against the
// recording C ABI of tests/cpp/abi_recorder.cpp: `estimator_trace <scenario>` prints every pb_* call the estimator makes (which call,
// into which slot, for every message), the estimator's own stderr messages in place, and a last line with its public counters and
// state.  tests/test_estimator_trace.py compares that output byte for byte with tests/golden/estimator_trace/<scenario>.txt, which
// were written from the header as it was BEFORE the estimator core was restructured -- a restructuring must not move a line.
// The header under test comes in through -DSHIM_HEADER='"..."' so that the same source compiles against an older header.
//
// Which scenario executes which branch of the estimator:
//   inorder_unfused   history_slots = 0, no fusion: the single-update path without a slot; an update older than the head is dropped;
//                     getHeadState / getMeasurementsLogLikelihood with nothing held (flushPending returns at once)
//   inorder_pairs     fuse_ins_legodo, every pair form: broadcast | host blocks with PB_R_DIAG / PB_R_DIAG_BROADCAST, with and without
//                     mask | device [6][B] block -> pb_step_legodo_split, with and without mask | a pair_kernel lambda; an INS step
//                     followed by something not fusible (position fix, orientation measurement, full R, IMU and measurement in different
//                     spaces, another INS step, make_measurement without pair_kernel); getHeadState while ONE update is held; a fused step that fails
//   inorder_triples   fuse_corrections: position_orient and position_yaw triples on a broadcast and on a host pair (per-filter and
//                     broadcast R, with mask); held = 2 with a deferred measurement resolved behind the held INS step (directly and as
//                     the first half of an RBISEitherUpdate); triples that do not fuse -- wrong index list, device-resident pair
//                     measurement, third update not an orientation measurement, full R, measurement / orientation in different spaces,
//                     per-filter R in another space; getHeadState while TWO updates are held; a fused triple that fails
//   ckpt_every1       history_checkpoint_every = 1: every update into its slot; late fixes -> restore + replay; equal time stamps;
//                     an update older than the window; the window sliding (clearHistoryBeforeUtime with checkpoints)
//   ckpt_every3_fuse  cadence 3 with fuse_ins_legodo: since_checkpoint += 2 per pair, pairs checkpointed behind their second half, late
//                     fixes that split pairs, a held INS step while the window slides
//   ckpt_pair_forms   every pair form and every near miss with checkpoints: which pairs count 2 towards the cadence and take the slot
//                     of their second half (the classification the fused-pair plan replaces)
//   ckpt_derived      only utime_history_span: pool and cadence derived; late fix, without and with fuse_ins_legodo
//   ckpt_exhausted    the pool exhausted: history_slots = 1 (reserve_slot returns -1: single update and pair) and 2 (the oldest part of
//                     the window is recycled)
//   slide_held        history_slots = 0: clearHistoryBeforeUtime with one and with two updates held
//   noroll            roll_forward = false: no deferred measurement; a deferred one behind the held INS step (ahead = that step);
//                     behind something else (flushPendingBefore); in front of an applied update (restore + replay); a make_measurement
//                     that fails; without fuse_ins_legodo (flushPendingBefore returns at once)
//   snapshot          snapshotPosteriorOf: a checkpointed update; the head; re-derived with the head parked in its own checkpoint and
//                     in a spare slot; no slot free; an unprocessed element; pendingImu
//   smooth_dense      EKFSmoothBackwardsPass with a checkpoint per update; fewer than two INS updates; history_slots = 0
//   smooth_sparse     cadence 3 and a loose head: stretches re-derived into the window; a second pass right after the first (the device
//                     no longer holds the newest posterior)
//   smooth_fused      ran_fused pairs re-applied fused (partner with and without a checkpoint of its own); a six-row pair_kernel
//                     partner that declines and is re-applied as two halves
//   smooth_ragged     the ragged overload: terminal slot, may_idle masks in host and in device memory, a step whose mask has no zero;
//                     too few free slots; a terminal slot that is free / out of range
//   smooth_bail_*     every bail site once (_save: saving the head, _restore: restoring a checkpoint, _pred_slot: setting the predicted
//                     slot, _pair: re-applying a fused pair, _update: re-applying an update, _step / _step_masked: the smoother steps,
//                     _head_back: putting the head back), and the next addUpdate, which finds device_head unknown
//   either            RBISEitherUpdate: first half into a slot, second in place on it; without a slot; replayed; appliesToNoFilter
//   yawlock           RBISYawLockUpdate in each mode: formed, then replayed by a late fix; appliesToNoFilter before and after
//   host_update       RBISHostUpdate with and without an `apply` mask, into a slot, replayed; a subclass that returns a wrong size
//   applies           RBISIndexedMeasurement::appliesToNoFilter: no mask, deferred, host masks, device mask (answer cached; a failing
//                     pb_mask_count)
//   create_fails      pb_history_reserve fails: the constructor's message (the process then exits with 1, as the reference's would)
#include <cinttypes>
#include <cstdio>
#include <deque>
#include <unistd.h>

#ifndef SHIM_HEADER
#define SHIM_HEADER "../../pronto_amd/csrc/mav_state_est.hpp"
#endif
#include SHIM_HEADER
#include "abi_recorder.h"

using namespace MavStateEst;
typedef RBISUpdateInterface U;

static void fill(std::vector<double> &v, double seed)
{
  for (size_t i = 0; i < v.size(); i++) v[i] = seed + 0.001 * (double) i;
}
static std::vector<double> vals(size_t k, double seed)
{
  std::vector<double> v(k);
  fill(v, seed);
  return v;
}

// one estimator with factories for the messages of a scenario; payloads that an update does not own live in `arena`
struct Sc {
  int B, n;
  BotParam param;
  std::unique_ptr<MavStateEstimator> est;
  std::deque<std::vector<double>> arena;
  std::deque<std::vector<uint8_t>> masks;
  std::vector<void *> devs;
  const double q[4] = { 7.6e-5, 0.01, 3e-10, 1e-8 };

  Sc(std::initializer_list<std::pair<const char *, const char *>> kv, int64_t span = 1000000, int B_ = 2, int n_ = 15) : B(B_), n(n_)
  {
    param.set("state_estimator.utime_history_span", (double) span);
    for (auto &p : kv) param.set(p.first, p.second);
    RBIS x0(n, B);
    RBIM P0(n, B);
    fill(x0.vec, 0.5);
    fill(P0.m, 0.25);
    est.reset(new MavStateEstimator(new RBISResetUpdate(x0, P0, U::reset, 0), &param, 0));
  }
  ~Sc()
  {
    state();
    for (void *p : devs) pb_free(est->ctx, p);
    est.reset();
  }
  void state() const
  {
    const MavStateEstimator &e = *est;
    printf("= replayed %jd dropped %jd fused_pairs %jd fused_triples %jd leg_kernel_pairs %jd rederived %jd smoother %jd %jd %jd status %d head_utime %jd history %zu free",
           (intmax_t) e.replayed_updates, (intmax_t) e.dropped_updates, (intmax_t) e.fused_pairs, (intmax_t) e.fused_triples, (intmax_t) e.leg_kernel_pairs,
           (intmax_t) e.rederived_posteriors, (intmax_t) e.smoother_reapplied_updates, (intmax_t) e.smoother_reapplied_pairs,
           (intmax_t) e.smoother_masked_steps, e.last_status, (intmax_t) e.head_utime, e.history.updateMap.size());
    std::vector<int> fs = e.free_slots;
    std::sort(fs.begin(), fs.end());
    for (int s : fs) printf(" %d", s);
    printf(" checkpoints");
    int pos = 0;
    for (auto &kv : e.history.updateMap) {
      auto it = e.checkpoint_of.find(kv.second);
      if (it != e.checkpoint_of.end()) printf(" %d->%d", pos, it->second);
      pos++;
    }
    printf("\n");
  }
  U *add(U *u, bool roll = true)
  {
    printf("# add %s t=%jd roll=%d\n", U::sensor_enum_string(u->sensor_id), (intmax_t) u->utime, (int) roll);
    est->addUpdate(u, roll);
    return u;
  }
  double *keep(size_t k, double seed) { arena.push_back(vals(k, seed)); return arena.back().data(); }
  uint8_t *keep_mask(std::vector<uint8_t> m) { masks.push_back(std::move(m)); return masks.back().data(); }
  std::vector<uint8_t> mask(int first = 1) const
  {
    std::vector<uint8_t> m((size_t) B, 0);
    for (int b = 0; b < B; b += 2) m[(size_t) b] = (uint8_t) first;
    return m;
  }
  void *dev(size_t bytes)
  {
    void *p = nullptr;
    pb_malloc(est->ctx, bytes, &p);
    devs.push_back(p);
    return p;
  }

  // 'b' one robot's message for every filter (PB_HOST_BROADCAST), 'h' a host block [7][B]
  RBISIMUProcessStep *imu(int64_t t, char form)
  {
    return new RBISIMUProcessStep(vals(form == 'b' ? 7 : (size_t) 7 * B, 1e-6 * t), q[0], q[1], q[2], q[3], t, form == 'b' ? PB_HOST_BROADCAST : PB_HOST);
  }
  // leg-odometry velocity measurement on {3,4,5}:  'b' broadcast | 'd' / 'D' host, R per filter, without / with mask | 'r' / 'R' host,
  // broadcast R | 'f' host, full R | 'v' / 'V' one device [6][B] block | 'k' deferred, with a pair kernel | 'K' the same, six rows |
  // 'm' deferred, make_measurement only | 'e' the same, and it fails | 'E' as 'k', make_measurement fails
  RBISIndexedMeasurement *vel(int64_t t, char form)
  {
    const double s = 2e-6 * t;
    const std::vector<int> idx = RBIS::velocityInds();
    switch (form) {
    case 'b': return new RBISIndexedMeasurement(idx, BatchArray(keep(3, s), PB_HOST_BROADCAST), keep(3, 0.02), PB_R_DIAG_BROADCAST, nullptr, U::legodo, t);
    case 'd': case 'D':
      return new RBISIndexedMeasurement(idx, vals((size_t) 3 * B, s), vals((size_t) 3 * B, 0.01), PB_R_DIAG, form == 'D' ? mask() : std::vector<uint8_t>(), U::legodo, t);
    case 'r': case 'R':
      return new RBISIndexedMeasurement(idx, vals((size_t) 3 * B, s), vals(3, 0.01), PB_R_DIAG_BROADCAST, form == 'R' ? mask() : std::vector<uint8_t>(), U::legodo, t);
    case 'f': return new RBISIndexedMeasurement(idx, vals((size_t) 3 * B, s), vals((size_t) 9 * B, 0.01), PB_R_FULL, {}, U::legodo, t);
    // the near misses of the pair forms: 'B' broadcast with a mask | 'g' broadcast with a per-filter R kind | 'c' host, R said to live
    // elsewhere | 'w' device z, broadcast R | 'W' device z, R in a block of its own
    case 'B': return new RBISIndexedMeasurement(idx, BatchArray(keep(3, s), PB_HOST_BROADCAST), keep(3, 0.02), PB_R_DIAG_BROADCAST, keep_mask(mask()), U::legodo, t);
    case 'g': return new RBISIndexedMeasurement(idx, BatchArray(keep(3, s), PB_HOST_BROADCAST), keep(3, 0.02), PB_R_DIAG, nullptr, U::legodo, t);
    case 'c': {
      auto *m = new RBISIndexedMeasurement(idx, vals((size_t) 3 * B, s), vals((size_t) 3 * B, 0.01), PB_R_DIAG, {}, U::legodo, t);
      m->cov_mem = PB_DEVICE;
      return m;
    }
    case 'w': return new RBISIndexedMeasurement(idx, BatchArray((double *) dev(sizeof(double) * 3 * B), PB_DEVICE), keep(3, 0.02), PB_R_DIAG_BROADCAST, nullptr, U::legodo, t);
    case 'W':
      return new RBISIndexedMeasurement(idx, BatchArray((double *) dev(sizeof(double) * 3 * B), PB_DEVICE), (double *) dev(sizeof(double) * 3 * B), PB_R_DIAG, nullptr, U::legodo, t);
    case 'v': case 'V': {
      double *p = (double *) dev(sizeof(double) * 6 * B);
      return new RBISIndexedMeasurement(idx, BatchArray(p, PB_DEVICE), p + (size_t) 3 * B, PB_R_DIAG, form == 'V' ? (uint8_t *) dev((size_t) B) : nullptr, U::legodo, t);
    }
    default: break;
    }
    // a measurement still to be made on the device (LegOdoHandler's joint / feet path): the lambdas log what they are asked
    const int rows = form == 'K' ? 6 : 3;
    double *p = (double *) dev(sizeof(double) * 2 * rows * B);
    uint8_t *mk = (uint8_t *) dev((size_t) B);
    auto *m = new RBISIndexedMeasurement(form == 'K' ? std::vector<int>{ 3, 4, 5, 0, 1, 2 } : idx, BatchArray(nullptr, PB_DEVICE), nullptr, PB_R_DIAG, nullptr, U::legodo, t);
    auto made = [m, p, mk, rows, this] {
      m->measurement = BatchArray(p, PB_DEVICE);
      m->measurement_cov = p + (size_t) rows * B;
      m->mask = mk;
    };
    const double *qq = q;
    if (form == 'k' || form == 'K' || form == 'E')
      m->pair_kernel = [made, p, mk, qq, t](pb_ctx *ctx, const RBISIMUProcessStep *step, bool keep_block) {
        printf("pair_kernel t=%jd imu=%jd keep=%d\n", (intmax_t) t, (intmax_t) step->utime, (int) keep_block);
        made();
        return pb_step_legodo_split(ctx, step->imu_block.p, step->imu_block.mem, p, mk, PB_DEVICE, qq);
      };
    m->make_measurement = [made, form, t](pb_ctx *, const RBISIMUProcessStep *ahead) {
      printf("make_measurement t=%jd ahead=%jd\n", (intmax_t) t, ahead ? (intmax_t) ahead->utime : (intmax_t) -1);
      made();
      return form == 'e' || form == 'E' ? (int) PB_ERR_ARG : (int) PB_OK;
    };
    return m;
  }
  RBISIndexedMeasurement *pos(int64_t t)
  {
    return new RBISIndexedMeasurement(RBIS::positionInds(), vals((size_t) 3 * B, 3e-6 * t), vals(3, 4e-4), PB_R_DIAG_BROADCAST, {}, U::gps, t);
  }
  // pose correction:  'h' host, broadcast R | 'H' host, R per filter, mask | 'b' broadcast | 'f' full R | 'x' orientation in another
  // space than the measurement | 'c' per-filter R in another space
  RBISIndexedPlusOrientationMeasurement *orient(int64_t t, std::vector<int> idx, char form)
  {
    const size_t m = idx.size(), Bz = (size_t) B;
    const double s = 4e-6 * t;
    switch (form) {
    case 'h': return new RBISIndexedPlusOrientationMeasurement(idx, vals(m * Bz, s), vals(m, 1e-3), PB_R_DIAG_BROADCAST, vals(4 * Bz, 0.5), {}, U::fovis, t);
    case 'H': return new RBISIndexedPlusOrientationMeasurement(idx, vals(m * Bz, s), vals(m * Bz, 1e-3), PB_R_DIAG, vals(4 * Bz, 0.5), mask(), U::scan_matcher, t);
    case 'f': return new RBISIndexedPlusOrientationMeasurement(idx, vals(m * Bz, s), vals(m * m * Bz, 1e-3), PB_R_FULL, vals(4 * Bz, 0.5), {}, U::fovis, t);
    case 'b':
      return new RBISIndexedPlusOrientationMeasurement(idx, BatchArray(keep(m, s), PB_HOST_BROADCAST), keep(m, 1e-3), PB_R_DIAG_BROADCAST,
                                                       BatchArray(keep(4, 0.5), PB_HOST_BROADCAST), nullptr, U::fovis, t);
    case 'x':
      return new RBISIndexedPlusOrientationMeasurement(idx, BatchArray(keep(m, s), PB_HOST_BROADCAST), keep(m, 1e-3), PB_R_DIAG_BROADCAST,
                                                       BatchArray(keep(4 * Bz, 0.5), PB_HOST), nullptr, U::fovis, t);
    default: {
      auto *o = new RBISIndexedPlusOrientationMeasurement(idx, BatchArray(keep(m * Bz, s), PB_HOST), keep(m * Bz, 1e-3), PB_R_DIAG,
                                                          BatchArray(keep(4 * Bz, 0.5), PB_HOST), nullptr, U::fovis, t);
      o->cov_mem = PB_DEVICE;
      return o;
    }
    }
  }
  // IMU step + velocity measurement at step k (utime k ms)
  void pair(int k, char imu_form, char vel_form)
  {
    add(imu(1000 * (int64_t) k, imu_form));
    add(vel(1000 * (int64_t) k, vel_form));
  }
  void head()
  {
    RBIS x;
    RBIM P;
    printf("# getHeadState\n");
    est->getHeadState(x, P);
    printf("# head utime %jd\n", (intmax_t) x.utime);
  }
  auto at(size_t position) { return std::next(est->history.updateMap.begin(), (long) position); }
};

static const std::vector<int> POS_ORIENT = { 9, 10, 11, 6, 7, 8 }, POS_YAW = { 9, 10, 11, 8 };
#define FUSE { "state_estimator.fuse_ins_legodo", "true" }
#define FUSE3 { "state_estimator.fuse_corrections", "1" }
#define SLOTS(s) { "state_estimator.history_slots", s }
#define EVERY(s) { "state_estimator.history_checkpoint_every", s }

static void inorder_unfused()
{
  Sc s({ SLOTS("0") });
  s.pair(1, 'b', 'b');
  s.add(s.pos(1000));
  s.pair(2, 'h', 'D');
  s.add(s.pos(1500));   // older than the head: discarded
  s.add(s.orient(2500, POS_ORIENT, 'h'));
  s.add(s.vel(3000, 'm'));
  s.add(s.vel(3000, 'k'));   // a pair kernel that never runs: no INS step in front, not fusing
  s.head();
  printf("# getMeasurementsLogLikelihood\n");
  s.est->getMeasurementsLogLikelihood();
}

static void inorder_pairs()
{
  Sc s({ SLOTS("0"), FUSE, { "state_estimator.fuse_corrections", "false" } });
  s.pair(1, 'b', 'b');
  s.pair(2, 'h', 'd');
  s.pair(3, 'h', 'D');
  s.pair(4, 'h', 'r');
  s.pair(5, 'h', 'R');
  s.pair(6, 'b', 'v');
  s.pair(7, 'h', 'V');
  s.pair(8, 'b', 'k');
  s.pair(9, 'h', 'K');
  s.add(s.imu(10000, 'b'));
  s.add(s.pos(10000));
  s.add(s.imu(11000, 'h'));
  s.add(s.orient(11000, POS_ORIENT, 'h'));
  s.pair(12, 'h', 'f');
  s.pair(13, 'b', 'd');
  s.pair(14, 'h', 'b');
  s.est->addUpdate(nullptr, true);          // ignored
  for (char form : { 'B', 'g', 'w', 'W' }) s.pair(140 + (form & 15), 'b', form);
  for (char form : { 'c', 'w', 'W' }) s.pair(160 + (form & 15), 'h', form);
  s.add(s.imu(215000, 'b'));
  s.add(s.imu(216000, 'b'));
  s.add(s.vel(216000, 'm'));
  s.add(s.imu(217000, 'b'));
  printf("# pendingImu %d\n", s.est->pendingImu() != nullptr);
  s.head();
  printf("# pendingImu %d\n", s.est->pendingImu() != nullptr);
  s.pair(218, 'b', 'b');
  rec_fail_call("pb_step_legodo", 1);
  s.pair(219, 'b', 'b');                     // the fused step fails: reported, the pair counts as applied
  U *last = s.add(s.imu(220000, 'b'));
  printf("# an INS step appliesToNoFilter %d\n", (int) last->appliesToNoFilter(s.est->ctx, s.B));
  rec_fail_call("pb_predict", 1);
  s.head();                                 // flushing the held step fails
}

static void inorder_triples()
{
  Sc s({ SLOTS("0"), FUSE, FUSE3 });
  s.pair(1, 'b', 'b');
  s.add(s.orient(1000, POS_ORIENT, 'b'));
  s.pair(2, 'h', 'D');
  s.add(s.orient(2000, POS_YAW, 'H'));
  s.pair(3, 'h', 'r');
  s.add(s.orient(3000, POS_ORIENT, 'h'));
  s.pair(4, 'b', 'b');
  s.add(s.orient(4000, POS_YAW, 'h'));
  s.pair(5, 'b', 'k');                      // held = 2: the odometry is made now, behind the held INS step
  s.add(s.orient(5000, POS_ORIENT, 'h'));   // a device-resident pair measurement: pairs, does not triple
  s.pair(6, 'b', 'b');
  s.add(s.orient(6000, RBIS::positionInds(), 'h'));   // wrong index list
  s.pair(7, 'b', 'v');
  s.add(s.orient(7000, POS_ORIENT, 'h'));
  s.pair(8, 'b', 'b');
  s.pair(9, 'b', 'b');                      // third = an INS step
  s.add(s.orient(9000, POS_ORIENT, 'f'));
  s.pair(10, 'b', 'b');
  s.add(s.orient(10000, POS_ORIENT, 'x'));
  s.pair(11, 'h', 'd');
  s.add(s.orient(11000, POS_YAW, 'c'));
  s.add(s.imu(12000, 'h'));
  s.add(new RBISEitherUpdate(s.vel(12000, 'K'), s.vel(12000, 'R')));
  s.add(s.pos(12000));
  s.pair(13, 'h', 'R');
  s.head();                                 // two updates held
  s.pair(14, 'b', 'b');
  s.add(s.pos(14500));
  s.add(s.imu(14700, 'b'));
  s.add(s.vel(14700, 'E'));                 // held = 2, and making its measurement fails
  s.add(s.pos(14800));
  rec_fail_call("pb_step_legodo_correct", 1);
  s.pair(15, 'b', 'b');
  s.add(s.orient(15000, POS_YAW, 'b'));     // the fused triple fails: reported, counts as applied
  s.add(s.pos(15500));
}

// T steps of IMU + leg odometry; a position fix stamped at step k arrives `delay` steps late when k % 4 == 2
static void run_late(Sc &s, int T, int delay, char imu_form, char vel_form)
{
  for (int k = 1; k <= T; k++) {
    s.pair(k, imu_form, vel_form);
    if (k - delay >= 1 && (k - delay) % 4 == 2) s.add(s.pos(1000 * (int64_t) (k - delay)));
  }
}

static void ckpt_every1()
{
  Sc s({ SLOTS("8"), EVERY("1") }, 3000);
  run_late(s, 8, 2, 'b', 'b');
  s.add(s.pos(2000));   // older than the window
  s.add(s.pos(8000));   // equal time stamps: behind the two updates of step 8
  s.add(s.pos(6000));
  rec_fail_call("pb_state_save", 1);
  s.pair(9, 'b', 'b');  // recording a checkpoint fails: the slot is kept, the status says so
  s.head();
}

static void ckpt_every3_fuse()
{
  Sc s({ SLOTS("6"), EVERY("3"), FUSE }, 4000);
  run_late(s, 9, 1, 'h', 'r');
  s.add(s.imu(10000, 'h'));
  s.add(s.pos(9000), true);   // late, in front of the held INS step
  s.pair(11, 'b', 'k');
  s.add(s.vel(11000, 'm'));
  rec_fail_call("pb_state_save", 1);
  for (int k = 12; k <= 14; k++) s.pair(k, 'b', 'b');   // recording a pair's checkpoint fails
  s.head();
}

// every pair form and near miss again, classified for a checkpoint slot (fusible_pair decides whether the pair counts 2)
static void ckpt_pair_forms()
{
  Sc s({ SLOTS("24"), EVERY("2"), FUSE });
  int k = 0;
  for (char form : { 'b', 'B', 'g', 'w', 'W', 'v', 'k', 'd', 'f' }) s.pair(++k, 'b', form);
  for (char form : { 'd', 'D', 'r', 'R', 'c', 'f', 'b', 'w', 'W', 'V', 'K' }) s.pair(++k, 'h', form);
  s.add(s.imu(1000 * ++k, 'h'));
  s.add(s.orient(1000 * k, POS_YAW, 'h'));
  s.add(s.imu(1000 * ++k, 'h'));
  s.add(new RBISEitherUpdate(s.vel(1000 * k, 'K'), s.vel(1000 * k, 'R')));
  s.head();
}

static void ckpt_derived()
{
  {
    Sc s({}, 30000);
    printf("# slots %d every %d\n", s.est->history_slots, s.est->checkpoint_every);
    run_late(s, 7, 3, 'b', 'b');
  }
  {
    Sc s({ FUSE, FUSE3 }, 2000);   // (fuse_corrections stays off with checkpoints)
    printf("# slots %d every %d fuse_corrections %d\n", s.est->history_slots, s.est->checkpoint_every, (int) s.est->fuse_corrections);
    run_late(s, 7, 1, 'b', 'v');
  }
  Sc s({ EVERY("0") }, 0);   // no span, no slots: in-order only; a cadence below 1 is 1
  printf("# slots %d every %d\n", s.est->history_slots, s.est->checkpoint_every);
  s.pair(1, 'b', 'b');
}

static void ckpt_exhausted()
{
  for (const char *slots : { "1", "2", "3" }) {
    Sc s({ SLOTS(slots), FUSE });
    s.pair(1, 'b', 'b');
    s.add(s.imu(2000, 'b'));
    s.add(s.pos(2000));
    s.add(s.pos(2500));
    s.pair(3, 'h', 'd');
    s.add(s.pos(1500));   // late: inside the window only where the pool kept it
    s.head();
  }
}

static void slide_held()
{
  {
    Sc s({ SLOTS("0"), FUSE });
    s.add(s.imu(1000, 'b'));
    s.add(s.imu(2000, 'b'));
    s.add(s.pos(2000));
    s.add(s.imu(3000, 'b'));
  }
  Sc s({ SLOTS("0"), FUSE, FUSE3 });
  s.pair(1, 'b', 'b');
  s.pair(2, 'b', 'b');
  s.add(s.pos(2000));
  s.pair(3, 'b', 'b');
}

static void noroll()
{
  {
    Sc s({ SLOTS("6"), EVERY("2"), FUSE });
    s.pair(1, 'b', 'b');
    s.add(s.pos(1000), false);            // no deferred measurement: stays unapplied
    s.add(s.imu(1000, 'b'), false);       // no measurement at all
    s.add(s.imu(2000, 'b'));              // applies the fix, is held itself
    s.add(s.vel(2000, 'k'), false);       // behind the held INS step: made now, slaved to the state after it
    s.add(s.imu(3000, 'b'));              // the pair runs (its pair kernel is gone: made already)
    s.add(s.pos(3000), false);
    rec_fail_call("pb_update_indexed", 1);
    s.add(s.vel(3000, 'K'), false);       // behind something else: what is pending in front of it is flushed
    s.pair(4, 'b', 'b');
    s.add(s.vel(3500, 'k'), false);       // in front of an applied update: restore + replay
    s.add(s.vel(4000, 'e'), false);       // its make_measurement fails
    s.add(s.imu(5000, 'b'));
    s.add(s.vel(4500, 'm'), false);       // late, but what follows it has not been applied
    s.head();
  }
  Sc s({ SLOTS("4"), EVERY("1") });
  s.pair(1, 'b', 'b');
  s.add(s.vel(2000, 'm'), false);
  s.add(s.vel(1500, 'm'), false);         // in front of the pending one
  s.add(s.vel(500, 'k'), false);          // in front of applied updates
  s.pair(3, 'b', 'b');
}

static void snapshot()
{
  Sc s({ SLOTS("7"), EVERY("3") });
  for (int k = 1; k <= 4; k++) s.pair(k, 'b', 'b');   // positions 0..8; checkpoints on 0, 3, 6
  auto snap = [&](size_t position, int slot) {
    printf("# snapshotPosteriorOf position %zu\n", position);
    const bool ok = s.est->snapshotPosteriorOf(s.at(position), slot);
    printf("# -> %d\n", (int) ok);
  };
  snap(3, 0);   // checkpointed
  snap(8, 1);   // the head
  snap(5, 0);   // re-derived, the head in a spare slot
  s.add(s.imu(5000, 'b'));   // position 9: checkpointed head
  snap(7, 1);   // re-derived, the head parked in its own checkpoint
  snap(9, 0);
  s.add(s.vel(5000, 'b'));
  rec_fail_call("pb_state_save", 1);
  snap(8, 0);   // parking the head fails
  rec_fail_call("pb_predict", 1);
  snap(8, 0);   // a re-applied update fails
  std::vector<int> taken;
  for (int slot; (slot = s.est->reserveSlot()) >= 0;) taken.push_back(slot);
  printf("# reserveSlot took %zu, then %d\n", taken.size(), s.est->reserveSlot());
  snap(8, 0);   // no slot to park the head in
  s.est->releaseSlot(taken.back());
  s.est->releaseSlot(taken.back());   // twice: ignored
  s.est->releaseSlot(99);
  s.est->releaseSlot(-1);
  rec_fail_call("pb_state_restore", 2);
  snap(4, 0);   // putting the head back fails
  snap(1, 0);
  s.add(s.pos(6000), false);
  snap(11, 0);  // not applied yet
  for (int slot : taken) s.est->releaseSlot(slot);
  Sc f({ SLOTS("4"), EVERY("2"), FUSE });
  for (int k = 1; k <= 3; k++) f.pair(k, 'b', 'b');
  f.add(f.imu(4000, 'b'));
  printf("# snapshotPosteriorOf the INS half of a pair, an INS step held -> %d\n", (int) f.est->snapshotPosteriorOf(f.at(3), 0));
}

static void smooth(Sc &s, bool ragged = false, int terminal = -1)
{
  printf("# EKFSmoothBackwardsPass%s terminal %d\n", ragged ? " ragged" : "", terminal);
  int steps;
  if (ragged)
    steps = s.est->EKFSmoothBackwardsPass(0.001, terminal, [](int64_t utime, int slot, const uint8_t *valid, int mem) {
      printf("on_smoothed utime=%jd slot=%d valid=%s mem=%d\n", (intmax_t) utime, slot, valid ? "set" : "NULL", mem);
    });
  else
    steps = s.est->EKFSmoothBackwardsPass(0.001, [](int64_t utime, int slot) { printf("on_smoothed utime=%jd slot=%d\n", (intmax_t) utime, slot); });
  printf("# -> %d steps\n", steps);
}

static void smooth_dense()
{
  {
    Sc s({ SLOTS("12"), EVERY("1") });
    s.pair(1, 'b', 'b');
    smooth(s);   // one INS update: nothing to smooth
    s.add(s.imu(2000, 'h'));
    s.pair(3, 'b', 'd');
    s.add(s.pos(3000));
    smooth(s);
    printf("# without a callback -> %d\n", s.est->EKFSmoothBackwardsPass(0.001, nullptr));
    printf("# ragged, without a callback -> %d\n", s.est->EKFSmoothBackwardsPass(0.001, -1, nullptr));
    std::vector<int> taken;
    while (s.est->free_slots.size() > 1) taken.push_back(s.est->reserveSlot());
    smooth(s);   // too few free slots, nothing to re-derive
    for (int slot : taken) s.est->releaseSlot(slot);
    Sc f({ SLOTS("12"), EVERY("1"), FUSE });   // fuse_ins_legodo, but no pair fused: nothing is missing
    f.pair(1, 'h', 'b');
    f.pair(2, 'h', 'b');
    f.add(f.pos(2000));
    smooth(f);
  }
  Sc s({ SLOTS("0") });
  s.pair(1, 'b', 'b');
  smooth(s);
}

static void smooth_sparse()
{
  Sc s({ SLOTS("12"), EVERY("3") });
  for (int k = 1; k <= 4; k++) s.pair(k, 'b', 'b');
  s.add(s.pos(4000));   // positions 0..9: checkpoints on 0, 3, 6, 9
  smooth(s);
  s.pair(5, 'b', 'b');  // a loose head
  smooth(s);
  smooth(s);            // the head was put back as a copy: device_head is unknown now
  printf("# snapshotPosteriorOf with device_head unknown -> %d\n", (int) s.est->snapshotPosteriorOf(s.at(1), 0));
  s.pair(6, 'b', 'b');
  std::vector<int> taken;
  while (s.est->free_slots.size() > 2) taken.push_back(s.est->reserveSlot());
  smooth(s);            // too few free slots with a loose head
  for (int slot : taken) s.est->releaseSlot(slot);
}

static void smooth_fused()
{
  Sc s({ SLOTS("14"), EVERY("3"), FUSE });
  s.pair(1, 'b', 'b');
  s.pair(2, 'h', 'R');
  s.pair(3, 'b', 'v');
  s.pair(4, 'h', 'K');   // its pair kernel runs once; the smoother re-applies the two halves
  s.add(s.pos(4000));
  s.pair(5, 'b', 'b');
  s.pair(6, 'b', 'k');
  s.add(s.imu(7000, 'b'));
  smooth(s);             // (flushes the held INS step: a loose head)
}

static void smooth_ragged()
{
  Sc s({ SLOTS("12"), EVERY("2") });
  uint8_t *dmask = (uint8_t *) s.dev(2);
  for (int k = 1; k <= 5; k++) {
    RBISIMUProcessStep *imu = s.imu(1000 * k, k == 2 ? 'b' : 'h');
    if (k == 1 || k == 3) { imu->valid_host = s.mask(); imu->may_idle = true; }
    if (k == 4) { imu->valid_dev = dmask; imu->may_idle = true; }
    if (k == 5) imu->valid_host = std::vector<uint8_t>(2, 1);   // a mask without a zero: the plain step
    s.add(imu);
    if (k != 3) s.add(s.vel(1000 * k, 'b'));
  }
  smooth(s, true);
  const int terminal = s.est->reserveSlot();
  smooth(s, true, terminal);   // (device_head unknown after the first pass, and nothing to re-derive it from: refused)
  s.pair(6, 'h', 'b');
  smooth(s, true, terminal);
  s.est->releaseSlot(terminal);
  s.pair(7, 'h', 'b');
  smooth(s, true, terminal);   // a free slot is no terminal slot
  smooth(s, true, 12);         // out of range
  std::vector<int> taken;
  while (s.est->free_slots.size() > 3) taken.push_back(s.est->reserveSlot());
  smooth(s, true);             // too few free slots
  for (int slot : taken) s.est->releaseSlot(slot);
}

// one bail site of the smoother: the kth call of fn fails during the pass
static void smooth_bail(const char *fn, int kth, bool ragged)
{
  Sc s({ SLOTS("12"), EVERY("4"), FUSE });
  s.pair(1, 'b', 'b');
  s.add(s.pos(1000));
  s.pair(2, 'b', 'b');
  RBISIMUProcessStep *imu = s.imu(3000, 'h');
  imu->valid_host = s.mask();
  imu->may_idle = true;
  s.add(imu);
  s.add(s.pos(3000));
  s.pair(4, 'b', 'b');
  s.add(s.pos(4000));
  s.est->flushPending();
  rec_fail_call(fn, kth);
  smooth(s, ragged);
  s.pair(5, 'b', 'b');   // afterwards: device_head unknown -> the next update restores a checkpoint and replays
  s.head();
}
static void smooth_bail_save() { smooth_bail("pb_state_save", 1, false); }
static void smooth_bail_restore() { smooth_bail("pb_state_restore", 1, false); }
static void smooth_bail_pred_slot() { smooth_bail("pb_set_pred_slot", 1, false); }
static void smooth_bail_pair() { smooth_bail("pb_step_legodo", 1, false); }
static void smooth_bail_update() { smooth_bail("pb_predict", 1, false); }
static void smooth_bail_step() { smooth_bail("pb_smooth_step", 2, false); }
static void smooth_bail_step_masked() { smooth_bail("pb_smooth_step_masked", 1, true); }
static void smooth_bail_head_back() { smooth_bail("pb_state_restore", 3, false); }

static void either()
{
  for (const char *slots : { "6", "0" }) {
    Sc s({ SLOTS(slots), EVERY("1") });
    s.pair(1, 'b', 'b');
    U *e = s.add(new RBISEitherUpdate(s.vel(1000, 'D'), s.vel(1000, 'R')));
    printf("# appliesToNoFilter %d\n", (int) e->appliesToNoFilter(s.est->ctx, s.B));
    auto *a = s.vel(2000, 'D'), *b = s.vel(2000, 'R');
    a->owned_mask.assign(2, 0);
    b->owned_mask.assign(2, 0);
    e = s.add(new RBISEitherUpdate(a, b));
    printf("# appliesToNoFilter %d\n", (int) e->appliesToNoFilter(s.est->ctx, s.B));
    rec_fail_call("pb_update_indexed", 1);
    s.add(new RBISEitherUpdate(s.vel(3000, 'D'), s.vel(3000, 'R')));   // the first half fails: the second does not run
    s.add(s.pos(500));    // late: replays both either-updates
  }
}

static void yawlock()
{
  Sc s({ SLOTS("8"), EVERY("2") }, 3000);
  const float joints[3] = { 0.1f, 0.2f, 0.3f };
  float *jdev = (float *) s.dev(sizeof(float) * 3 * 2);
  auto pool = std::make_shared<DevicePool>(s.est->ctx, s.est->ctx_alive, sizeof(double) * 6 * 2 + 2 * 2);
  std::vector<RBISYawLockUpdate *> ups;
  for (int mode = 0; mode < 3; mode++) {
    s.pair(mode + 1, 'b', 'b');
    bool fresh;
    void *blk = pool->get(fresh);
    printf("# block fresh %d\n", (int) fresh);
    const msgs_joint_ref j = { mode == 1 ? jdev : joints, 3, mode == 1 ? PB_DEVICE : PB_HOST_BROADCAST };
    auto *u = new RBISYawLockUpdate(mode, j, (uint8_t) (mode != 2), 0.01 * mode, 1e-4, 2e-4, std::make_shared<DeviceBlock>(pool, blk), 1000 * (mode + 1) + 500);
    printf("# appliesToNoFilter before it is formed %d\n", (int) u->appliesToNoFilter(s.est->ctx, s.B));
    s.add(u);
    ups.push_back(u);
  }
  rec_set_mask_count(0);
  printf("# appliesToNoFilter %d, again %d\n", (int) ups[0]->appliesToNoFilter(s.est->ctx, s.B), (int) ups[0]->appliesToNoFilter(s.est->ctx, s.B));
  rec_set_mask_count(1);
  printf("# appliesToNoFilter %d\n", (int) ups[1]->appliesToNoFilter(s.est->ctx, s.B));
  rec_fail_call("pb_mask_count", 2);
  printf("# appliesToNoFilter %d, then %d\n", (int) ups[2]->appliesToNoFilter(s.est->ctx, s.B), (int) ups[2]->appliesToNoFilter(s.est->ctx, s.B));
  s.add(s.pos(500));    // late: every yaw-lock update is re-applied from the measurement it kept
  rec_fail_call("pb_update_indexed_orient", 1);
  s.add(s.pos(600));    // ... and the replay of the first one with an orientation row fails
  rec_fail_call("pb_yawlock_set_gyro", 1);
  bool fresh;
  void *blk = pool->get(fresh);
  const msgs_joint_ref j = { joints, 3, PB_HOST_BROADCAST };
  s.add(new RBISYawLockUpdate(2, j, 1, 0.0, 1e-4, 2e-4, std::make_shared<DeviceBlock>(pool, blk), 5000));
  s.add(s.pos(3600));   // the window slides: blocks go back to the pool
  blk = pool->get(fresh);
  printf("# block fresh %d\n", (int) fresh);
  DeviceBlock back(pool, blk);
  rec_fail_call("pb_malloc", 1);
  DevicePool other(s.est->ctx, s.est->ctx_alive, 64);
  printf("# a failing pb_malloc gives %s\n", other.get(fresh) == nullptr ? "NULL" : "a block");
}

struct Altimeter : RBISHostUpdate {
  bool wrong_size;
  Altimeter(int64_t t, bool wrong = false) : RBISHostUpdate(altimeter, t), wrong_size(wrong) {}
  using RBISHostUpdate::updateFilter;
  void updateFilter(const RBIS &prior, const RBIM &prior_cov, double ll) override
  {
    printf("user updateFilter utime=%jd z=%.17g P=%.17g ll=%.17g\n", (intmax_t) prior.utime, prior(11, 0), prior_cov(11, 11, 0), ll);
    posterior_state(11, 0) = 0.5 * prior(11, 0);
    posterior_covariance(11, 11, 0) = 0.5 * prior_cov(11, 11, 0);
    loglikelihood = ll - 1;
    if (wrong_size) posterior_state = RBIS(21, 1);
  }
};

static void host_update()
{
  Sc s({ SLOTS("6"), EVERY("1") }, 1000000, 3);
  s.pair(1, 'b', 'b');
  s.add(new Altimeter(1500));
  auto *masked = new Altimeter(2000);
  masked->apply = { 1, 0, 1 };
  s.add(masked);
  s.add(s.pos(1200));   // late: both are replayed
  s.add(new Altimeter(3000, true));
  rec_fail_call("pb_get_head", 1);
  s.add(new Altimeter(4000));
}

static void applies()
{
  Sc s({ SLOTS("0") });
  auto ask = [&](RBISIndexedMeasurement *m) {
    printf("# appliesToNoFilter %d, again %d\n", (int) m->appliesToNoFilter(s.est->ctx, s.B), (int) m->appliesToNoFilter(s.est->ctx, s.B));
    delete m;
  };
  ask(s.vel(1000, 'd'));   // no mask
  ask(s.vel(1000, 'k'));   // deferred
  ask(s.vel(1000, 'D'));   // a host mask with a one
  auto *m = s.vel(1000, 'R');
  m->owned_mask.assign(2, 0);
  ask(m);                  // a host mask of zeros
  rec_set_mask_count(0);
  ask(s.vel(1000, 'V'));   // a device mask: pb_mask_count, once
  rec_set_mask_count(2);
  ask(s.vel(1000, 'V'));
  rec_fail_call("pb_mask_count", 1);
  ask(s.vel(1000, 'V'));   // the count fails: "applies", not cached
}

static void create_fails()
{
  rec_fail_call("pb_history_reserve", 1);
  Sc s({ SLOTS("4") });
}

static const struct { const char *name; void (*run)(); } SCENARIOS[] = {
  { "inorder_unfused", inorder_unfused }, { "inorder_pairs", inorder_pairs }, { "inorder_triples", inorder_triples },
  { "ckpt_every1", ckpt_every1 }, { "ckpt_every3_fuse", ckpt_every3_fuse }, { "ckpt_pair_forms", ckpt_pair_forms },
  { "ckpt_derived", ckpt_derived },
  { "ckpt_exhausted", ckpt_exhausted }, { "slide_held", slide_held }, { "noroll", noroll }, { "snapshot", snapshot },
  { "smooth_dense", smooth_dense }, { "smooth_sparse", smooth_sparse }, { "smooth_fused", smooth_fused },
  { "smooth_ragged", smooth_ragged }, { "smooth_bail_save", smooth_bail_save }, { "smooth_bail_restore", smooth_bail_restore }, { "smooth_bail_pred_slot", smooth_bail_pred_slot },
  { "smooth_bail_pair", smooth_bail_pair }, { "smooth_bail_update", smooth_bail_update }, { "smooth_bail_step", smooth_bail_step },
  { "smooth_bail_step_masked", smooth_bail_step_masked }, { "smooth_bail_head_back", smooth_bail_head_back }, { "either", either }, { "yawlock", yawlock },
  { "host_update", host_update }, { "applies", applies }, { "create_fails", create_fails },
};

int main(int argc, char **argv)
{
  // one unbuffered stream: the estimator's stderr messages land between the calls that surround them
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
  fprintf(stderr, "usage: estimator_trace --list | <scenario>\n");
  return 2;
}
