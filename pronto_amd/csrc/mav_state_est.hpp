// mav_state_est.hpp -- the estimator core of the host-side C++ mirror of Pronto's update-object API for B filters at once: what the
// reference keeps in rbis.hpp, rbis_update_interface.hpp, update_history.hpp and mav_state_est.hpp / .cpp.  Header-only on top of the C ABI
// (include/pronto_batch.h) and the standard library, nothing else:
//
//   BotParam + the bot_* stand-ins, RBIS / RBIM / BatchArray, DevicePool / DeviceBlock
//   RBISUpdateInterface + RBISResetUpdate / RBISIMUProcessStep / RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement /
//   RBISHostUpdate / RBISEitherUpdate / RBISYawLockUpdate             state-estimator/src/mav_state_est/rbis_update_interface.hpp:8-120
//   updateHistory                                                      update_history.hpp:12-36
//   MavStateEstimator::addUpdate / getHeadState / getMeasurementsLogLikelihood / EKFSmoothBackwardsPass   mav_state_est.hpp:10-25, .cpp:28-189
//
// This is the code that decides which pb_* call runs, and into which checkpoint slot, for every message.  It talks to the device through
// the C ABI only, so tests/cpp/estimator_trace.cpp runs it on the CPU against a recording stand-in for those functions and
// tests/test_estimator_trace.py pins every decision to the traces under tests/golden/estimator_trace/.  The message types, the IMU front
// end, the sensor handlers, the publishers and the log player are in mav_state_est_batch.hpp, which includes this header.
#pragma once


#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pronto_batch.h"

namespace MavStateEst {

// ---------------------------------------------------------------------------------------------------------------
// libbot stand-ins (bot_param, bot_core math) -- same names and semantics as the calls in the reference
// ---------------------------------------------------------------------------------------------------------------
struct BotParam {
  std::map<std::string, std::string> kv;
  void set(const std::string &k, const std::string &v) { kv[k] = v; }
  void set(const std::string &k, double v)
  {
    char b[64];
    snprintf(b, sizeof b, "%.17g", v);
    kv[k] = b;
  }
  // "-O key=value|key=value" overrides (fusion.cpp:98-99, lcm_front_end.cpp:62-68)
  void applyOverrides(const std::string &s)
  {
    size_t p = 0;
    while (p < s.size()) {
      size_t e = s.find('|', p);
      if (e == std::string::npos) e = s.size();
      std::string kvp = s.substr(p, e - p);
      size_t eq = kvp.find('=');
      if (eq != std::string::npos) kv[kvp.substr(0, eq)] = kvp.substr(eq + 1);
      p = e + 1;
    }
  }
};

// the value of an optional key, NULL when it is not set
inline const std::string *bot_param_find(BotParam *p, const char *key)
{
  auto it = p->kv.find(key);
  return it == p->kv.end() ? nullptr : &it->second;
}
inline const std::string &bot_param_get_raw_or_fail(BotParam *p, const char *key)
{
  const std::string *v = bot_param_find(p, key);
  if (v == nullptr) {
    fprintf(stderr, "ERROR: BotParam: could not get param value for key '%s'\n", key);
    exit(1);  // libbot bot_param_get_*_or_fail behaviour
  }
  return *v;
}
inline double bot_param_get_double_or_fail(BotParam *p, const char *key) { return atof(bot_param_get_raw_or_fail(p, key).c_str()); }
inline int64_t bot_param_get_int_or_fail(BotParam *p, const char *key) { return atoll(bot_param_get_raw_or_fail(p, key).c_str()); }
inline bool bot_param_get_boolean_or_fail(BotParam *p, const char *key)
{
  const std::string &v = bot_param_get_raw_or_fail(p, key);
  return v == "true" || v == "1" || v == "True";
}
inline std::string bot_param_get_str_or_fail(BotParam *p, const char *key) { return bot_param_get_raw_or_fail(p, key); }
// optional keys (this build's additions, and keys the reference reads with a default): the default when the key is not set
inline int bot_param_get_int_or(BotParam *p, const char *key, int dflt)
{
  const std::string *v = bot_param_find(p, key);
  return v ? atoi(v->c_str()) : dflt;
}
inline double bot_param_get_double_or(BotParam *p, const char *key, double dflt)
{
  const std::string *v = bot_param_find(p, key);
  return v ? atof(v->c_str()) : dflt;
}
// an optional flag: off unless the key is set to "true" or "1" (NOT "True", which bot_param_get_boolean_or_fail also takes)
inline bool bot_param_get_flag(BotParam *p, const char *key)
{
  const std::string *v = bot_param_find(p, key);
  return v != nullptr && (*v == "true" || *v == "1");
}
// "x, y, z" or "[x, y, z]": libbot's bot_param_get_double_array_or_fail
inline void bot_param_get_double_array_or_fail(BotParam *p, const char *key, double *out, int len)
{
  const std::string &v = bot_param_get_raw_or_fail(p, key);
  const char *c = v.c_str();
  for (int i = 0; i < len; i++) {
    while (*c == ' ' || *c == '[' || *c == ',') c++;
    char *end = nullptr;
    out[i] = strtod(c, &end);
    if (end == c) {
      fprintf(stderr, "ERROR: BotParam: '%s' does not hold %d numbers\n", key, len);
      exit(1);
    }
    c = end;
  }
}
inline double bot_sq(double a) { return a * a; }
inline double bot_to_radians(double d) { return d * (M_PI / 180.0); }

struct BotTrans {
  double rot_quat[4] = { 1, 0, 0, 0 };
  double trans_vec[3] = { 0, 0, 0 };
  bool isIdentityRotation() const { return rot_quat[0] == 1 && rot_quat[1] == 0 && rot_quat[2] == 0 && rot_quat[3] == 0; }
};
// libbot bot_quat_rotate_to (restated in-tree at pronto-utils/src/pronto_complementary/complementary_test.cpp:49-59)
inline void bot_quat_rotate_to(const double rot[4], const double v[3], double r[3])
{
  double ab = rot[0] * rot[1], ac = rot[0] * rot[2], ad = rot[0] * rot[3];
  double nbb = -rot[1] * rot[1], bc = rot[1] * rot[2], bd = rot[1] * rot[3];
  double ncc = -rot[2] * rot[2], cd = rot[2] * rot[3], ndd = -rot[3] * rot[3];
  r[0] = 2 * ((ncc + ndd) * v[0] + (bc - ad) * v[1] + (ac + bd) * v[2]) + v[0];
  r[1] = 2 * ((ad + bc) * v[0] + (nbb + ndd) * v[1] + (cd - ab) * v[2]) + v[1];
  r[2] = 2 * ((bd - ac) * v[0] + (ab + cd) * v[1] + (nbb + ncc) * v[2]) + v[2];
}
inline void bot_trans_apply_vec(const BotTrans *t, const double v[3], double r[3])
{
  bot_quat_rotate_to(t->rot_quat, v, r);
  r[0] += t->trans_vec[0]; r[1] += t->trans_vec[1]; r[2] += t->trans_vec[2];
}

// ---------------------------------------------------------------------------------------------------------------
// batched RBIS / RBIM (rbis.hpp:19-123): host containers, SoA with the filter index fastest
// ---------------------------------------------------------------------------------------------------------------
struct RBIS {
  enum { angular_velocity_ind = 0, velocity_ind = 3, chi_ind = 6, position_ind = 9, acceleration_ind = 12,
         basic_num_states = 15, gyro_bias_ind = 15, accel_bias_ind = 18, rbis_num_states = 21 };
  int n = 0, B = 0;
  int64_t utime = 0;
  std::vector<double> vec;   // [n][B]
  std::vector<double> quat;  // [4][B]  (w,x,y,z)
  RBIS() {}
  RBIS(int n_states, int batch) : n(n_states), B(batch), vec((size_t) n_states * batch, 0.0), quat((size_t) 4 * batch, 0.0)
  {
    for (int b = 0; b < B; b++) quat[b] = 1.0;
  }
  double &operator()(int i, int b) { return vec[(size_t) i * B + b]; }
  double operator()(int i, int b) const { return vec[(size_t) i * B + b]; }
  double &q(int i, int b) { return quat[(size_t) i * B + b]; }
  double q(int i, int b) const { return quat[(size_t) i * B + b]; }
  static std::vector<int> positionInds() { return { 9, 10, 11 }; }
  static std::vector<int> velocityInds() { return { 3, 4, 5 }; }
  static std::vector<int> chiInds() { return { 6, 7, 8 }; }
  static std::vector<int> angularVelocityInds() { return { 0, 1, 2 }; }
};

struct RBIM {
  int n = 0, B = 0;
  std::vector<double> m;  // [n*n][B], column-major per filter (Map<RBIM>, rbis.cpp:300)
  RBIM() {}
  RBIM(int n_states, int batch) : n(n_states), B(batch), m((size_t) n_states * n_states * batch, 0.0) {}
  double &operator()(int r, int c, int b) { return m[((size_t) c * n + r) * B + b]; }
  double operator()(int r, int c, int b) const { return m[((size_t) c * n + r) * B + b]; }
};

// a batched array handed over by a message: pointer + where it lives
struct BatchArray {
  const double *p = nullptr;
  int mem = PB_HOST;
  BatchArray() {}
  BatchArray(const double *ptr, int m) : p(ptr), mem(m) {}
};
// What the handlers share when they take a host message over (the update objects own their host payloads, see below):
// the values per row -- one per filter, or one for all (PB_HOST_BROADCAST) --
inline size_t batch_per(int mem, int B) { return mem == PB_HOST_BROADCAST ? 1 : (size_t) B; }
// an owned copy of `rows` host rows of a message array,
inline std::vector<double> own_rows(const BatchArray &a, size_t rows, int B) { return std::vector<double>(a.p, a.p + rows * batch_per(a.mem, B)); }
// and of a host mask [B]: none without a mask, and none for one robot's message (it is for every filter)
inline std::vector<uint8_t> own_mask(const uint8_t *mask, int mem, int B)
{
  return (mask != nullptr && mem == PB_HOST) ? std::vector<uint8_t>(mask, mask + B) : std::vector<uint8_t>();
}
// Hamilton product r = a * b (w,x,y,z); r must not be a or b
inline void quat_mult(const double a[4], const double b[4], double r[4])
{
  r[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  r[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  r[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  r[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
// A handler's report of a failed library call: "<who>: <pb_last_error>" on stderr.  Yields nullptr, so that a handler that gives the
// message up writes `return pb_report(...)`; the sibling ends the program like every bad configuration (libbot's *_or_fail behaviour).
inline std::nullptr_t pb_report(const char *who, pb_ctx *ctx)
{
  fprintf(stderr, "%s: %s\n", who, pb_last_error(ctx));
  return nullptr;
}
[[noreturn]] inline void pb_report_exit(const char *who, pb_ctx *ctx)
{
  pb_report(who, ctx);
  exit(1);
}

class MavStateEstimator;

// Device memory that an update object OWNS (the reference's update objects own their measurement; here a measurement that
// was formed on the device -- FovisHandler's T1 = T0 * delta -- must stay what it was when the history re-applies the
// update after a late arrival).  Blocks of one size are recycled through a pool shared by the handler and its updates;
// `alive` is the estimator's lifetime token: device memory is only released while the context still exists.
struct DevicePool {
  pb_ctx *ctx;
  std::shared_ptr<bool> alive;
  size_t bytes;
  std::vector<void *> free_;
  DevicePool(pb_ctx *c, std::shared_ptr<bool> a, size_t b) : ctx(c), alive(std::move(a)), bytes(b) {}
  ~DevicePool()
  {
    if (alive && *alive)
      for (void *p : free_) pb_free(ctx, p);
  }
  // One hipMalloc per NEW block, on purpose: while the history window is still filling (the first utime_history_span of a run, ~500
  // blocks for the reference's 1 s) a few-MB hipMalloc measures ~10 us and hides behind the step it feeds, whereas slabs of many
  // blocks stall the message that asks for them (a 1 GiB hipMalloc: up to 30 ms, profiles/r04_shim_sweep.txt).
  void *get(bool &fresh)
  {
    fresh = free_.empty();
    void *p = nullptr;
    if (!fresh) {
      p = free_.back();
      free_.pop_back();
    } else if (pb_malloc(ctx, bytes, &p) != PB_OK) {
      p = nullptr;
    }
    return p;
  }
};
struct DeviceBlock {
  std::shared_ptr<DevicePool> pool;
  void *p;
  DeviceBlock(std::shared_ptr<DevicePool> pl, void *ptr) : pool(std::move(pl)), p(ptr) {}
  ~DeviceBlock() { if (p) pool->free_.push_back(p); }  // stream order makes the reuse safe: every consumer was enqueued before
  DeviceBlock(const DeviceBlock &) = delete;
  DeviceBlock &operator=(const DeviceBlock &) = delete;
};
// a block of `pool` as an update owns it (back into the pool with its last owner), or null: pb_malloc failed.  fresh: never used before
inline std::shared_ptr<DeviceBlock> take_block(const std::shared_ptr<DevicePool> &pool, bool *fresh = nullptr)
{
  bool is_fresh = false;
  void *p = pool->get(is_fresh);
  if (fresh != nullptr) *fresh = is_fresh;
  return p != nullptr ? std::make_shared<DeviceBlock>(pool, p) : nullptr;
}

// ---------------------------------------------------------------------------------------------------------------
// update objects (rbis_update_interface.hpp)
// ---------------------------------------------------------------------------------------------------------------
class RBISUpdateInterface {
public:
  typedef enum {
    ins, gps, vicon, laser, laser_gpf, scan_matcher, optical_flow, reset, invalid, rgbd, fovis, legodo, pose_meas,
    altimeter, airspeed, sideslip, init_message, viewer, yawlock
  } sensor_enum;
  int64_t utime;
  sensor_enum sensor_id;
  RBISUpdateInterface(sensor_enum sensor_id_, int64_t utime_) : utime(utime_), sensor_id(sensor_id_) {}
  virtual ~RBISUpdateInterface() {}
  // Applies this update to the estimator's device-resident posterior (prior = previous posterior,
  // mav_state_est.cpp:55-57).  Returns a pb_status; the posterior/loglikelihood stay on the device.
  virtual int updateFilter(pb_ctx *ctx) = 0;
  // true: this update changes NO filter of the batch -- the message for which the reference's handler returns NULL, so that
  // nothing enters the history (rbis_legodo_update.cpp:242-255).  A batched handler whose per-filter validity is decided on the
  // device cannot know that when it returns; the question is asked lazily (pb_mask_count synchronises), only where the difference
  // is observable: FovisHandler's history.updateMap.lower_bound look-up skips such updates.
  virtual bool appliesToNoFilter(pb_ctx * /*ctx*/, int /*B*/) { return false; }
  static const char *sensor_enum_string(sensor_enum s)
  {
    static const char *names[] = { "ins", "gps", "vicon", "laser", "laser_gpf", "scan_matcher", "optic_flow", "reset",
                                   "invalid", "rgbd", "fovis", "legodo", "pose_meas", "altimeter", "airspeed",
                                   "sideslip", "init_message", "viewer", "yawlock" };
    return names[(int) s];
  }
};

class RBISResetUpdate : public RBISUpdateInterface {
public:
  RBIS reset_state;
  RBIM reset_cov;
  RBISResetUpdate(const RBIS &state, const RBIM &cov, sensor_enum sensor_id_, int64_t utime)
      : RBISUpdateInterface(sensor_id_, utime), reset_state(state), reset_cov(cov) {}
  int updateFilter(pb_ctx *ctx) override
  {
    return pb_reset(ctx, reset_state.vec.data(), reset_state.quat.data(), reset_cov.m.data(), 0, PB_HOST);
  }
};

class RBISIMUProcessStep : public RBISUpdateInterface {
public:
  // gyro xyz | accelerometer xyz | dt as ONE block [7][B] (body frame), owned when built on the host
  std::vector<double> owned;
  std::shared_ptr<DeviceBlock> owned_dev;  // a block made on the device (InsHandler's device path: pb_ins_body_block)
  // [B] DEVICE or NULL: 0 = this filter has NO IMU message in this step (independent log segments; the reference's handler returned
  // NULL for it).  Whoever takes this step hands the mask to the library first (announce): the step is then a no-op for it.
  const uint8_t *valid_dev = nullptr;
  void announce(pb_ctx *ctx) const { if (valid_dev) pb_set_imu_valid(ctx, valid_dev); }
  // the same mask of a step built from HOST messages (InsHandler::build: such a filter's block entry has dt = 0), an owned copy for as
  // long as the step lives in the history: EKFSmoothBackwardsPass reads it (the step itself never announces it)
  std::vector<uint8_t> valid_host;
  // some filter MAY have no message in this step: its mask has a zero, or it lives on the device and was never seen on the host
  bool may_idle = false;
  // this step's mask and where it lives (PB_HOST / PB_DEVICE); NULL = every filter has a message
  const uint8_t *stepMask(int &mem) const
  {
    mem = valid_host.empty() ? PB_DEVICE : PB_HOST;
    return valid_host.empty() ? valid_dev : valid_host.data();
  }
  BatchArray imu_block;
  double q_gyro, q_accel, q_gyro_bias, q_accel_bias;
  // set by MavStateEstimator when this step last ran fused with the update behind it (fuse_ins_legodo): its own posterior then has no
  // checkpoint, and EKFSmoothBackwardsPass re-derives it by re-applying the pair with a predicted slot (pb_set_pred_slot)
  bool ran_fused = false;
  RBISIMUProcessStep(BatchArray imu_block_, double q_gyro_, double q_accel_, double q_gyro_bias_, double q_accel_bias_,
                     int64_t utime)
      : RBISUpdateInterface(ins, utime), imu_block(imu_block_), q_gyro(q_gyro_), q_accel(q_accel_),
        q_gyro_bias(q_gyro_bias_), q_accel_bias(q_accel_bias_) {}
  RBISIMUProcessStep(std::vector<double> &&block, double q_gyro_, double q_accel_, double q_gyro_bias_,
                     double q_accel_bias_, int64_t utime, int mem = PB_HOST)  // PB_HOST_BROADCAST: block is [7]
      : RBISUpdateInterface(ins, utime), owned(std::move(block)), imu_block(owned.data(), mem), q_gyro(q_gyro_),
        q_accel(q_accel_), q_gyro_bias(q_gyro_bias_), q_accel_bias(q_accel_bias_) {}
  int updateFilter(pb_ctx *ctx) override
  {
    const double q[4] = { q_gyro, q_accel, q_gyro_bias, q_accel_bias };
    announce(ctx);
    return pb_predict(ctx, imu_block.p, q, imu_block.mem);
  }
};

class RBISIndexedMeasurement : public RBISUpdateInterface {
public:
  std::vector<int> index;
  std::vector<double> owned_z, owned_R;
  std::vector<uint8_t> owned_mask;
  std::shared_ptr<DeviceBlock> owned_dev;  // device-resident z / quat / mask this update owns (FovisHandler)
  BatchArray measurement;           // [m][B]
  const double *measurement_cov;    // per r_kind
  int r_kind, cov_mem;
  const uint8_t *mask = nullptr;    // [B]; 0 = this filter's handler returned NULL (lcm_front_end.hpp:156)
  // A measurement that is still to be MADE on the device from the head state (leg kinematic odometry, LegOdoHandler): either
  // together with the INS step in front of it -- pair_kernel: that step, the odometry slaved to the state after it and this
  // update in ONE kernel (pb_step_legodo_joints / _feet; keep = write the measurement block out for later re-applications) --
  // or on its own right before this update is applied (make_measurement).  Whichever runs first clears both: the odometry
  // advances once, a history replay re-applies the measurement it left in `measurement` / `mask`.
  // make_measurement(ctx, ahead): ahead != NULL = slaved to the state AFTER that (still pending) INS step -- what the estimator
  // calls when it has to hold the pair back or was told not to roll forward, so that the handler's inputs are consumed before
  // control returns to the caller (they are only valid until the next message).
  std::function<int(pb_ctx *, const RBISIMUProcessStep *, bool keep)> pair_kernel;
  std::function<int(pb_ctx *, const RBISIMUProcessStep *ahead)> make_measurement;
  bool deferred() const { return (bool) make_measurement; }
  // run the deferred odometry now (no-op when there is none); afterwards `measurement` / `mask` hold its result
  int resolve(pb_ctx *ctx, const RBISIMUProcessStep *ahead)
  {
    if (!make_measurement) return PB_OK;
    const int rc = make_measurement(ctx, ahead);
    make_measurement = nullptr;
    pair_kernel = nullptr;
    return rc;
  }
  RBISIndexedMeasurement(const std::vector<int> &index_, BatchArray measurement_, const double *measurement_cov_,
                         int r_kind_, const uint8_t *mask_, sensor_enum sensor_id_, int64_t utime)
      : RBISUpdateInterface(sensor_id_, utime), index(index_), measurement(measurement_),
        measurement_cov(measurement_cov_), r_kind(r_kind_), cov_mem(measurement_.mem), mask(mask_) {}
  // host-built measurement: takes ownership of z [m][B], R (per r_kind) and mask
  RBISIndexedMeasurement(const std::vector<int> &index_, std::vector<double> &&z, std::vector<double> &&R, int r_kind_,
                         std::vector<uint8_t> &&mask_, sensor_enum sensor_id_, int64_t utime)
      : RBISUpdateInterface(sensor_id_, utime), index(index_), owned_z(std::move(z)), owned_R(std::move(R)),
        owned_mask(std::move(mask_)), measurement(owned_z.data(), PB_HOST), measurement_cov(owned_R.data()),
        r_kind(r_kind_), cov_mem(PB_HOST), mask(owned_mask.empty() ? nullptr : owned_mask.data()) {}
  int updateFilter(pb_ctx *ctx) override
  {
    const int rc = resolve(ctx, nullptr);
    if (rc != PB_OK) return rc;
    return pb_update_indexed(ctx, (int) index.size(), index.data(), measurement.p, measurement_cov, r_kind, mask,
                             measurement.mem);
  }
  bool appliesToNoFilter(pb_ctx *ctx, int B) override
  {
    if (mask == nullptr || deferred()) return false;  // (a deferred measurement has no mask yet: not applied, not empty)
    if (empty_known_) return empty_;
    int n = 1;
    if (measurement.mem == PB_DEVICE) {
      if (pb_mask_count(ctx, mask, &n) != PB_OK) return false;
    } else {
      n = 0;
      for (int b = 0; b < B; b++) n += mask[b] != 0;
    }
    empty_known_ = true;
    return empty_ = (n == 0);
  }
private:
  bool empty_known_ = false, empty_ = false;
};

class RBISIndexedPlusOrientationMeasurement : public RBISIndexedMeasurement {
public:
  std::vector<double> owned_q;
  BatchArray orientation;  // [4][B]
  RBISIndexedPlusOrientationMeasurement(const std::vector<int> &index_, BatchArray measurement_,
                                        const double *measurement_cov_, int r_kind_, BatchArray orientation_,
                                        const uint8_t *mask_, sensor_enum sensor_id_, int64_t utime)
      : RBISIndexedMeasurement(index_, measurement_, measurement_cov_, r_kind_, mask_, sensor_id_, utime),
        orientation(orientation_) {}
  RBISIndexedPlusOrientationMeasurement(const std::vector<int> &index_, std::vector<double> &&z, std::vector<double> &&R,
                                        int r_kind_, std::vector<double> &&quat, std::vector<uint8_t> &&mask_,
                                        sensor_enum sensor_id_, int64_t utime)
      : RBISIndexedMeasurement(index_, std::move(z), std::move(R), r_kind_, std::move(mask_), sensor_id_, utime),
        owned_q(std::move(quat)), orientation(owned_q.data(), PB_HOST) {}
  int updateFilter(pb_ctx *ctx) override
  {
    return pb_update_indexed_orient(ctx, (int) index.size(), index.data(), measurement.p, measurement_cov, r_kind,
                                    orientation.p, mask, measurement.mem);
  }
};
// The two measurements built from a HOST message in `mem` -- PB_HOST, or PB_HOST_BROADCAST: one robot's z [m] (and quat [4]) for every
// filter.  The update owns z, R (per r_kind; a per-filter R lives where z does), the mask and the quaternion.
inline RBISIndexedMeasurement *hostIndexedMeasurement(const std::vector<int> &index, std::vector<double> z, std::vector<double> R, int r_kind,
                                                      std::vector<uint8_t> mask, int mem, RBISUpdateInterface::sensor_enum sensor, int64_t utime)
{
  auto *u = new RBISIndexedMeasurement(index, std::move(z), std::move(R), r_kind, std::move(mask), sensor, utime);
  u->measurement.mem = mem;
  if (r_kind != PB_R_DIAG_BROADCAST) u->cov_mem = mem;
  return u;
}
// (every handler that measures an orientation has one diagonal R for all filters: PB_R_DIAG_BROADCAST)
inline RBISIndexedPlusOrientationMeasurement *hostIndexedPlusOrientationMeasurement(const std::vector<int> &index, std::vector<double> z, std::vector<double> R_diag,
                                                                                    std::vector<double> quat, std::vector<uint8_t> mask, int mem,
                                                                                    RBISUpdateInterface::sensor_enum sensor, int64_t utime)
{
  auto *u = new RBISIndexedPlusOrientationMeasurement(index, std::move(z), std::move(R_diag), PB_R_DIAG_BROADCAST, std::move(quat), std::move(mask), sensor, utime);
  u->measurement.mem = u->orientation.mem = mem;
  return u;
}

// An update written against the REFERENCE's contract (rbis_update_interface.hpp:14-35):
//     virtual void updateFilter(const RBIS & prior_state, const RBIM & prior_cov, double prior_loglikelihood) = 0;
// "must fill posterior_state, posterior_covariance, loglikelihood".  This is what a third-party RBISUpdateInterface subclass looks
// like (RBISOpticalFlowMeasurement, rbis_update_interface.hpp:128-154; RBISLaserGPFMeasurement::updateFilter,
// gpf/rbis_gpf_update.cpp:28-76): user arithmetic on ONE filter's state.  It runs here on the SLOW path, documented as such: the
// batch's head comes to the host (pb_get_head), the user's updateFilter is called once per filter with single-filter RBIS / RBIM
// (B = 1 containers: prior_state(i, 0), prior_state.q(i, 0), prior_cov(r, c, 0)), and the posteriors go back (pb_set_head) --
// two PCIe crossings of the whole state per update, 2 x 126 MB at 64k 15-state filters.  The built-in updates never take it.
// apply[b] = false (optional mask, like a handler's NULL return for filter b) leaves filter b's head as it is.
class RBISHostUpdate : public RBISUpdateInterface {
public:
  RBIS posterior_state;          // single-filter containers, filled by the user's updateFilter
  RBIM posterior_covariance;
  double loglikelihood = 0;
  std::vector<uint8_t> apply;    // [B] or empty (= every filter)
  RBISHostUpdate(sensor_enum sensor_id_, int64_t utime_) : RBISUpdateInterface(sensor_id_, utime_) {}
  virtual void updateFilter(const RBIS &prior_state, const RBIM &prior_cov, double prior_loglikelihood) = 0;
  int updateFilter(pb_ctx *ctx) final
  {
    const int n = pb_n_states(ctx), B = pb_batch(ctx);
    std::vector<double> vec((size_t) n * B), quat((size_t) 4 * B), cov((size_t) n * n * B), ll((size_t) B);
    int rc = pb_get_head(ctx, 0, B, vec.data(), quat.data(), cov.data(), ll.data(), PB_HOST);
    if (rc != PB_OK) return rc;
    RBIS prior(n, 1);
    RBIM prior_cov(n, 1);
    for (int b = 0; b < B; b++) {
      if (!apply.empty() && !apply[(size_t) b]) continue;
      for (int i = 0; i < n; i++) prior.vec[(size_t) i] = vec[(size_t) i * B + b];
      for (int i = 0; i < 4; i++) prior.quat[(size_t) i] = quat[(size_t) i * B + b];
      for (int i = 0; i < n * n; i++) prior_cov.m[(size_t) i] = cov[(size_t) i * B + b];
      prior.utime = utime;
      posterior_state = prior;               // (a subclass that forgets a member leaves the prior there, not garbage)
      posterior_covariance = prior_cov;
      loglikelihood = ll[(size_t) b];
      updateFilter(prior, prior_cov, ll[(size_t) b]);
      if (posterior_state.n != n || posterior_state.B != 1 || posterior_covariance.n != n || posterior_covariance.B != 1) return PB_ERR_ARG;
      for (int i = 0; i < n; i++) vec[(size_t) i * B + b] = posterior_state.vec[(size_t) i];
      for (int i = 0; i < 4; i++) quat[(size_t) i * B + b] = posterior_state.quat[(size_t) i];
      for (int i = 0; i < n * n; i++) cov[(size_t) i * B + b] = posterior_covariance.m[(size_t) i];
      ll[(size_t) b] = loglikelihood;
    }
    return pb_set_head(ctx, vec.data(), quat.data(), cov.data(), ll.data(), PB_HOST);
  }
};

// Two updates with complementary per-filter masks that together are ONE update of the reference (each filter takes
// exactly one branch): used where the reference changes the measurement dimension per message (LegOdoCommon's
// pos_and_lin_rate -> lin_rate fallback, rbis_legodo_common.cpp:118-122).  If the first half wrote its posterior into a
// checkpoint slot, the second half works in place on that slot.
class RBISEitherUpdate : public RBISUpdateInterface {
public:
  RBISUpdateInterface *first, *second;
  RBISEitherUpdate(RBISUpdateInterface *a, RBISUpdateInterface *b) : RBISUpdateInterface(a->sensor_id, a->utime), first(a), second(b) {}
  ~RBISEitherUpdate() override { delete first; delete second; }
  int updateFilter(pb_ctx *ctx) override
  {
    int rc = first->updateFilter(ctx);
    if (rc != PB_OK) return rc;
    const int slot = pb_head_slot(ctx);
    if (slot >= 0) pb_set_output_slot(ctx, slot);
    return second->updateFilter(ctx);
  }
  bool appliesToNoFilter(pb_ctx *ctx, int B) override { return first->appliesToNoFilter(ctx, B) && second->appliesToNoFilter(ctx, B); }
};

// the joint positions of one message as an update takes them over
struct msgs_joint_ref {
  const float *p;
  int n_rows, mem;
};

// What YawLockHandler::processMessage returns (rbis_yawlock_update.cpp:193-228): an RBISIndexedMeasurement /
// RBISIndexedPlusOrientationMeasurement whose content depends on each filter's own head pose and yaw-lock state, so it is FORMED on
// the device, when the update is first applied (MavStateEstimator::addUpdate: the head is then the state at its place in the
// history), by the kernel that also applies it -- pb_step_yawlock_joints.  The update owns the joint positions of its message
// and, from then on, the measurement that was applied: z [2][B], quaternion [4][B], masks [2][B] in one device block.  A
// delayed-measurement replay re-applies THAT (pb_update_indexed_orient / pb_update_indexed with the two masks); the state machine
// never runs twice for one message.
class RBISYawLockUpdate : public RBISUpdateInterface {
public:
  int mode;                            // 0 yawbias, 1 yaw, 2 yawbias_yaw
  std::vector<float> joint_position;   // one robot's raw joint positions (PB_HOST_BROADCAST), or empty: joint_dev
  const float *joint_dev = nullptr;    // [rows][B] device block of the caller (valid until the update has been applied)
  int n_rows, joints_mem;
  uint8_t standing;                    // what the status handler last decided
  double gyro_z;                       // body-frame gyro z of the last IMU message (insHandler)
  double R[2];                         // the diagonal of the mode's row set
  double r_bias;
  std::shared_ptr<DeviceBlock> kept;   // z | quat | masks
  bool formed = false;
  RBISYawLockUpdate(int mode_, const msgs_joint_ref &j, uint8_t standing_, double gyro_z_, double r_bias_, double r_yaw_,
                    std::shared_ptr<DeviceBlock> block, int64_t utime)
      : RBISUpdateInterface(yawlock, utime), mode(mode_), n_rows(j.n_rows), joints_mem(j.mem), standing(standing_), gyro_z(gyro_z_),
        r_bias(r_bias_), kept(std::move(block))
  {
    if (j.mem == PB_HOST_BROADCAST) joint_position.assign(j.p, j.p + j.n_rows);
    else joint_dev = j.p;
    R[0] = mode == 1 ? r_yaw_ : r_bias_;
    R[1] = r_yaw_;
  }
  double *z(int B) const { (void) B; return (double *) kept->p; }
  double *quat(int B) const { return (double *) kept->p + 2 * (size_t) B; }
  uint8_t *masks(int B) const { return (uint8_t *) ((double *) kept->p + 6 * (size_t) B); }
  int updateFilter(pb_ctx *ctx) override
  {
    const int B = pb_batch(ctx);
    if (!formed) {
      formed = true;
      int rc = pb_yawlock_set_standing(ctx, &standing, PB_HOST_BROADCAST);
      if (rc == PB_OK) rc = pb_yawlock_set_gyro(ctx, &gyro_z, PB_HOST_BROADCAST);
      if (rc != PB_OK) return rc;
      return pb_step_yawlock_joints(ctx, utime, nullptr, nullptr, n_rows, joint_position.empty() ? joint_dev : joint_position.data(), joints_mem,
                                    z(B), quat(B), masks(B));
    }
    // a replay: the kept measurement, the row set with the orientation and / or the bias row alone (complementary masks; if the
    // first half wrote into a checkpoint slot, the second works in place on it, as RBISEitherUpdate)
    int rc = PB_OK;
    if (mode != 0) {
      const int idx[2] = { mode == 1 ? 8 : 17, 8 };
      rc = pb_update_indexed_orient(ctx, mode == 1 ? 1 : 2, idx, z(B), R, PB_R_DIAG_BROADCAST, quat(B), masks(B), PB_DEVICE);
      if (rc != PB_OK || mode == 1) return rc;
      const int slot = pb_head_slot(ctx);
      if (slot >= 0) pb_set_output_slot(ctx, slot);
    }
    const int idx1[1] = { 17 };
    return pb_update_indexed(ctx, 1, idx1, z(B), &r_bias, PB_R_DIAG_BROADCAST, masks(B) + B, PB_DEVICE);
  }
  // the batch-wide idle message (no filter gets an update): known once the measurement has been formed
  bool appliesToNoFilter(pb_ctx *ctx, int B) override
  {
    if (!formed) return false;
    if (empty_known_) return empty_;
    int n0 = 1, n1 = 1;
    if (pb_mask_count(ctx, masks(B), &n0) != PB_OK || pb_mask_count(ctx, masks(B) + B, &n1) != PB_OK) return false;
    empty_known_ = true;
    return empty_ = (n0 + n1 == 0);
  }
private:
  bool empty_known_ = false, empty_ = false;
};

// ---------------------------------------------------------------------------------------------------------------
// updateHistory + MavStateEstimator (update_history.hpp:12-36, mav_state_est.hpp / .cpp:12-96)
//
// The reference stores every update's posterior inside the update object; a delayed measurement is inserted at
// its timestamp and everything from there on is re-applied (mav_state_est.cpp:28-80).  Here the posterior of the
// whole batch lives on the device, so the history keeps, per update, an optional CHECKPOINT slot
// (pb_state_save) instead; a replay restores the newest checkpoint at or before the insertion point and re-applies
// the updates after it.  checkpoint_every = 1 is the reference's "posterior per update"; larger values trade HBM
// (73 MB per slot for 64k 15-state filters) for longer replays.  With history_slots = 0 the estimator is in-order
// only: an update older than the head is discarded like one older than the history (update_history.cpp:28-39).
// Updates in the history own their host payloads; device payloads they point to must outlive the window.
// ---------------------------------------------------------------------------------------------------------------
class updateHistory {
public:
  typedef std::multimap<int64_t, RBISUpdateInterface *> historyMap;
  typedef historyMap::iterator historyMapIterator;
  typedef std::pair<int64_t, RBISUpdateInterface *> historyPair;
  historyMap updateMap;
  ~updateHistory()
  {
    for (auto &kv : updateMap) delete kv.second;  // update_history.cpp:9-14
  }
};

class MavStateEstimator {
public:
  int64_t utime_history_span;
  pb_ctx *ctx = nullptr;
  std::shared_ptr<bool> ctx_alive = std::make_shared<bool>(false);  // lifetime token for device memory owned elsewhere
  int n = 0, B = 0;
  int64_t head_utime = 0;
  int last_status = PB_OK;
  updateHistory history;
  updateHistory::historyMapIterator unprocessed_updates_start;
  // checkpoint bookkeeping (this build's addition; keys state_estimator.history_slots / history_checkpoint_every)
  int history_slots = 0, checkpoint_every = 1, since_checkpoint = 0;
  std::map<RBISUpdateInterface *, int> checkpoint_of;
  std::vector<int> free_slots;
  RBISUpdateInterface *device_head = nullptr;  // the update whose posterior the device currently holds
  int64_t replayed_updates = 0;                // statistics: updates re-applied because of late arrivals
  int64_t dropped_updates = 0;                 // updates discarded as too old (update_history.cpp:28-39)
  bool derived_history_ = false;               // history_slots / checkpoint cadence were derived from utime_history_span
  // state_estimator.fuse_ins_legodo = true (this build's addition, off by default; works with and without checkpoints): an INS process step is held back
  // until the next update arrives; if that is a velocity measurement on {3,4,5} with a diagonal R (LegOdoCommon's
  // lin_rate) both run as ONE fused kernel (pb_step_legodo: one state round trip instead of two -- 21.7 us instead of
  // 20.2 + 23.6 us at 64k filters).  Only the posterior after the pair exists then, so this is for replays nobody
  // observes between the two messages; with posterior checkpoints (history_slots > 0) the pair is checkpointed as one
  // update behind its second half (the backward smoother needs every INS posterior and refuses to run with it).
  // Anything that reads the device (getHeadState, FovisHandler) flushes the held step first.
  bool fuse_ins_legodo = false;
  int64_t fused_pairs = 0;
  // state_estimator.fuse_corrections = true (with fuse_ins_legodo): the fused pair is held back one more message; if
  // that is a FovisHandler position_orient (idx 9,10,11,6,7,8) or ScanMatcherHandler position_yaw (idx 9,10,11,8)
  // measurement with a diagonal R, all THREE updates run as one kernel and one state round trip
  // (pb_step_legodo_correct; reference seam: rbis_fovis_update.cpp:299-305, sensor_handlers.cpp:709-722).
  bool fuse_corrections = false;
  int64_t fused_triples = 0;
  int64_t leg_kernel_pairs = 0;  // fused pairs whose leg odometry ran inside the step kernel (pb_step_legodo_joints / _feet)

  MavStateEstimator(RBISResetUpdate *init_state, BotParam *param, int device = 0, int n_snapshots = 2)
  {
    utime_history_span = bot_param_get_int_or_fail(param, "state_estimator.utime_history_span");
    // The reference re-orders and re-applies ANY update inside utime_history_span (update_history.cpp:16-42,
    // mav_state_est.cpp:28-80).  Here that needs posterior checkpoints on the device, so a configuration that only sets
    // utime_history_span (every reference .cfg) gets a default pool: 32 slots, spaced so that they cover the span at an
    // assumed two updates per millisecond (1 kHz IMU + leg odometry).  state_estimator.history_slots = 0 asks explicitly
    // for the in-order-only estimator (no checkpoints; an update older than the head is counted in dropped_updates and
    // discarded) -- the throughput configuration of the benchmarks.
    if (bot_param_find(param, "state_estimator.history_slots") == nullptr && utime_history_span > 0) {
      const int64_t expected = std::min<int64_t>(utime_history_span / 500 + 1, 1 << 20);
      history_slots = (int) std::min<int64_t>(32, expected + 2);
      checkpoint_every = (int) std::max<int64_t>(1, (expected + history_slots - 3) / std::max(1, history_slots - 2));
      derived_history_ = true;
    } else {
      history_slots = bot_param_get_int_or(param, "state_estimator.history_slots", 0);
      checkpoint_every = 1;
    }
    checkpoint_every = bot_param_get_int_or(param, "state_estimator.history_checkpoint_every", checkpoint_every);
    if (checkpoint_every < 1) checkpoint_every = 1;
    fuse_ins_legodo = bot_param_get_flag(param, "state_estimator.fuse_ins_legodo");
    // (with posterior checkpoints a fused PAIR is checkpointed as one update, behind its second half; the three-message
    // fusion is for the in-order-only estimator)
    fuse_corrections = fuse_ins_legodo && history_slots == 0 && bot_param_get_flag(param, "state_estimator.fuse_corrections");
    n = init_state->reset_state.n;
    B = init_state->reset_state.B;
    int rc = pb_create(&ctx, n, B, device, n_snapshots);
    if (rc == PB_OK && history_slots > 0) rc = pb_history_reserve(ctx, history_slots);
    if (rc != PB_OK) {
      fprintf(stderr, "MavStateEstimator: %s\n", pb_last_error(rc == PB_OK ? nullptr : ctx));
      exit(1);  // the reference's constructor cannot fail softly either (bot_param_get_int_or_fail)
    }
    *ctx_alive = true;
    for (int i = history_slots - 1; i >= 0; i--) free_slots.push_back(i);
    last_status = init_state->updateFilter(ctx);  // "apply update from zero... should reset the state" (:16)
    head_utime = init_state->utime;
    pb_set_utime(ctx, head_utime);
    history.updateMap.insert(updateHistory::historyPair(init_state->utime, init_state));  // update_history.cpp:5-8
    device_head = init_state;
    if (history_slots > 0) {
      save_checkpoint(init_state);
      // A replay never re-applies the first element of the history (it starts from that element's checkpoint), so the [n][B] and
      // [n][n][B] host arrays of the initial reset are given back here: freeing them when the window first slides past the
      // initial state (126 MB at 64k x 15 states, 243 MB at 21) stalls that one message for 16-41 ms.
      if (slot_of(init_state) >= 0) {
        init_state->reset_state = RBIS();
        init_state->reset_cov = RBIM();
      }
    }
    unprocessed_updates_start = history.updateMap.end();
  }
  ~MavStateEstimator()
  {
    // updates may own device memory of this context: release them first, then the context
    for (auto &kv : history.updateMap) delete kv.second;
    history.updateMap.clear();
    *ctx_alive = false;
    pb_destroy(ctx);
  }
  MavStateEstimator(const MavStateEstimator &) = delete;
  MavStateEstimator &operator=(const MavStateEstimator &) = delete;

  // Takes ownership of `update` (the reference's history deletes it, update_history.cpp:12,36,52).
  void addUpdate(RBISUpdateInterface *update, bool roll_forward)
  {
    if (update == nullptr) return;
    auto &map = history.updateMap;
    // update_history.cpp:16-42: insert by time (equal keys keep arrival order); too old -> discard
    const int64_t oldest = (history_slots > 0) ? map.begin()->first : head_utime;
    if (update->utime < oldest) {
      fprintf(stderr, "error: update type %s had timestamp %jd, which was before the first in history (%jd)\ndiscarding update!\n",
              RBISUpdateInterface::sensor_enum_string(update->sensor_id), (intmax_t) update->utime, (intmax_t) oldest);
      delete update;
      dropped_updates++;
      return;
    }
    const auto old_start = unprocessed_updates_start;
    auto added_it = map.insert(map.end(), updateHistory::historyPair(update->utime, update));
    if (unprocessed_updates_start == map.end() || added_it->first < unprocessed_updates_start->first)
      unprocessed_updates_start = added_it;                                   // mav_state_est.cpp:33-40
    if (!roll_forward) {
      // a measurement that is still to be made from the handler's inputs is made NOW (those inputs are the caller's and only
      // valid until its next message): slaved to the state after the INS step in front of it when that is the one held back.
      // The update ITSELF stays unapplied (roll_forward = false).
      auto *m = deferredMeasurement(update);
      if (m == nullptr || !m->deferred()) return;
      // a late arrival in front of an update that HAS been applied: the state its odometry reads is the one at its place in the
      // history, so it takes the restore-checkpoint + replay path below like a rolled-forward update
      auto after = std::next(added_it);
      bool next_applied = after != map.end();
      for (auto it = old_start; next_applied && it != map.end(); ++it)
        if (it == after) next_applied = false;
      if (!next_applied) {
        RBISIMUProcessStep *ahead = nullptr;
        if (holding_ == 1 && added_it != map.begin()) {
          auto prev = std::prev(added_it);
          if (prev == unprocessed_updates_start) ahead = as_imu(prev->second);
        }
        if (ahead == nullptr) flushPendingBefore(added_it);   // (what is pending IN FRONT of it, never the new element)
        const int rc = m->resolve(ctx, ahead);
        if (rc != PB_OK) last_status = rc;
        return;
      }
    }

    // The prior of the first unprocessed update is the posterior of the update before it (:45-57).  If the device
    // does not hold that posterior (late arrival), restore the newest checkpoint at or before it and replay.
    auto prev_it = unprocessed_updates_start;
    --prev_it;
    auto current_it = unprocessed_updates_start;
    if (prev_it->second != device_head) {
      const auto origin = checkpoint_at_or_before(prev_it);
      last_status = pb_state_restore(ctx, slot_of(origin->second));
      current_it = std::next(origin);
      for (auto it = current_it; it != unprocessed_updates_start; ++it) replayed_updates++;
      for (auto it = unprocessed_updates_start; it != map.end(); ++it)
        if (it != added_it) replayed_updates++;
      // checkpoints after the insertion point are stale now
      for (auto it = current_it; it != map.end(); ++it) drop_checkpoint(it->second);
      since_checkpoint = 0;
    }
    int held = 0;
    while (current_it != map.end()) {
      RBISUpdateInterface *u = current_it->second;
      if (auto *imu = fuse_ins_legodo ? as_imu(u) : nullptr) {
        auto nxt = std::next(current_it);
        if (nxt == map.end() && !flushing_) {  // newest element: hold it back until the next update shows up
          held = 1;
          break;
        }
        // how the step and the update behind it run as one launch, decided ONCE: what reserves a slot for the pair below is what runs it
        const PairPlan pair = nxt != map.end() ? plan_pair(imu, nxt->second) : PairPlan();
        if (fuse_corrections && pair) {
          auto third = std::next(nxt);
          if (third == map.end() && !flushing_) {  // the pair is complete: wait for what follows it
            // (its measurement is made now, slaved to the state after the held INS step: the handler's inputs do not
            // outlive this call)
            const int rrc = pair.m->resolve(ctx, imu);
            if (rrc != PB_OK) last_status = rrc;
            held = 2;
            break;
          }
          int rc = PB_OK;
          if (third != map.end() && run_fused3(imu, pair, third->second, rc)) {
            if (rc != PB_OK) {
              last_status = rc;
              fprintf(stderr, "MavStateEstimator::addUpdate: fused ins+legodo+correction step failed: %s\n", pb_last_error(ctx));
            }
            imu->ran_fused = false;   // (triples: no checkpoints, no smoother pass)
            fused_triples++;
            device_head = third->second;
            head_utime = third->second->utime;
            current_it = ++third;
            continue;
          }
        }
        if (pair) {
          apply_step(nxt->second, imu, pair);
          current_it = ++nxt;
          continue;
        }
      }
      apply_step(u, nullptr, PairPlan());
      ++current_it;
    }
    pb_set_utime(ctx, head_utime);
    holding_ = held;
    clearHistoryBeforeUtime(head_utime - utime_history_span);                 // :72-77
    unprocessed_updates_start = held ? current_it : map.end();
  }

  // the INS step fuse_ins_legodo is holding back, when it is the ONLY pending update (nullptr otherwise): a handler whose
  // measurement depends on the head state (leg kinematic odometry) can ask the device for the state "after that step"
  // instead of flushing it, so that the pair still runs as one fused kernel
  RBISIMUProcessStep *pendingImu()
  {
    if (!fuse_ins_legodo || holding_ != 1 || unprocessed_updates_start == history.updateMap.end()) return nullptr;
    auto it = unprocessed_updates_start;
    auto *imu = as_imu(it->second);
    if (imu == nullptr || ++it != history.updateMap.end()) return nullptr;
    return imu;
  }
  // apply an INS step that fuse_ins_legodo is holding back (no-op otherwise)
  void flushPending() { flushPendingBefore(history.updateMap.end()); }

  // the same for the pending updates IN FRONT of `stop` only; `stop` and what follows it stay unprocessed
  void flushPendingBefore(updateHistory::historyMapIterator stop)
  {
    if (!fuse_ins_legodo || unprocessed_updates_start == history.updateMap.end() || unprocessed_updates_start == stop) return;
    flushing_ = true;
    for (auto it = unprocessed_updates_start; it != stop && it != history.updateMap.end(); ++it) {
      int rc = it->second->updateFilter(ctx);
      if (rc != PB_OK) last_status = rc;
      device_head = it->second;
      head_utime = it->second->utime;
    }
    flushing_ = false;
    holding_ = 0;
    pb_set_utime(ctx, head_utime);
    unprocessed_updates_start = stop;
  }

  void getHeadState(RBIS &head_state, RBIM &head_cov)
  {
    flushPending();
    head_state = RBIS(n, B);
    head_cov = RBIM(n, B);
    last_status = pb_get_head(ctx, 0, B, head_state.vec.data(), head_state.quat.data(), head_cov.m.data(), nullptr, PB_HOST);
    head_state.utime = head_utime;
  }
  std::vector<double> getMeasurementsLogLikelihood()
  {
    flushPending();
    std::vector<double> ll(B);
    last_status = pb_get_head(ctx, 0, B, nullptr, nullptr, nullptr, ll.data(), PB_HOST);
    return ll;
  }

  // (position, quaternion) of the posterior of the update at `it` into device snapshot slot `snap_slot`: what the reference
  // reads as lower_it->second->posterior_state (rbis_fovis_update.cpp:196-206) -- every update keeps its posterior there.
  // Here only every checkpoint_every-th update (and never the INS half of a fused pair) has a saved posterior; for the others
  // it is re-derived: the nearest earlier checkpoint into the context's own array, the updates up to `it` re-applied, the
  // snapshot taken, and the head put back.  Costs at most checkpoint_every re-applied updates per call; FovisHandler calls it
  // once per keyframe change.  false: `it` has not been applied yet, or no slot is free to park the head in.
  int64_t rederived_posteriors = 0;
  bool snapshotPosteriorOf(updateHistory::historyMapIterator it, int snap_slot)
  {
    auto &map = history.updateMap;
    flushPending();
    for (auto u = unprocessed_updates_start; u != map.end(); ++u)
      if (u == it) return false;  // (added without roll_forward: no posterior exists yet)
    const int ck = slot_of(it->second);
    if (ck >= 0) return (last_status = pb_snapshot_from_slot(ctx, snap_slot, ck)) == PB_OK;
    if (it->second == device_head) return (last_status = pb_snapshot(ctx, snap_slot)) == PB_OK;
    // where the head goes meanwhile: its own checkpoint if it has one, else a spare slot
    int park = device_head ? slot_of(device_head) : -1;
    const bool park_is_spare = park < 0;
    if (park_is_spare) {
      if (free_slots.empty()) return false;
      park = free_slots.back();
      free_slots.pop_back();
      if ((last_status = pb_state_save(ctx, park)) != PB_OK) return false;
    }
    const auto origin = checkpoint_at_or_before(it);
    int rc = pb_state_restore(ctx, slot_of(origin->second));
    for (auto u = std::next(origin); rc == PB_OK; ++u) {
      rc = u->second->updateFilter(ctx);
      if (u == it) break;
    }
    if (rc == PB_OK) rc = pb_snapshot(ctx, snap_slot);
    const int rc2 = pb_state_restore(ctx, park);   // the head again (a copy in the context's own array)
    if (park_is_spare) free_slots.push_back(park);
    pb_set_utime(ctx, head_utime);
    rederived_posteriors++;
    if (rc != PB_OK || rc2 != PB_OK) last_status = rc != PB_OK ? rc : rc2;
    return rc == PB_OK && rc2 == PB_OK;
  }

  // EKFSmoothBackwardsPass (mav_state_est.cpp:98-189): walk the history backwards; at every INS update k apply
  // ekfSmoothingStep with  next_pred = posterior of INS_{k+1},  next = smoothed posterior of step k+1 (for the newest
  // step: its last measurement's posterior),  cur = posterior of the last measurement that followed INS_k (or INS_k's
  // own when none did).  The reference reads these posteriors out of its update objects, which keep them by value; here a
  // posterior exists where an update has a CHECKPOINT slot.  With a checkpoint on every update of the window
  // (history_checkpoint_every = 1) the pass only reads; with sparser checkpoints -- the only way a long window of a big batch
  // fits the device: 64k 21-state filters are 135 MB per posterior -- it re-derives what is missing, stretch by stretch from the
  // newest: the updates between two checkpoints are re-applied from the older one into a window of free slots (checkpoint and
  // recompute: history_slots >= window / every + every + 3 instead of one per update; pb_smooth_log is the same idea for device
  // streams).  The smoothed posteriors are bit for bit those of the all-checkpoints pass.
  // The reference overwrites the updates' posteriors with the smoothed ones for later republishing; here
  // on_smoothed(utime of INS_k, slot) is called newest-first with a slot that holds the smoothed posterior until the next call
  // (pb_get_slot reads it; pb_state_restore(slot) + getHeadState too).  Returns the number of steps, -1 on an error.
  // With fuse_ins_legodo an INS update that ran fused with the update behind it has no posterior of its own (the pair kernel keeps the
  // prediction in registers): the pass treats it as missing and re-applies the PAIR in one fused launch that writes the prediction
  // into the INS update's window slot (pb_set_pred_slot) and the pair's posterior into the partner's (pb_set_output_slot) -- never
  // into an existing checkpoint: when the partner has one, into one more window slot.
  int64_t smoother_reapplied_updates = 0;   // statistics: updates re-applied to re-derive posteriors that had no checkpoint
  int64_t smoother_reapplied_pairs = 0;     // ... of which fused INS + leg-odometry pairs, re-applied as one launch (each counts once)
  int64_t smoother_masked_steps = 0;        // smoother steps that also ran pb_slot_select (ragged overload: a tick some filter sat out)
  int EKFSmoothBackwardsPass(double dt, const std::function<void(int64_t, int)> &on_smoothed)
  {
    return smooth_pass(dt, -1, false, [&](int64_t utime, int slot, const uint8_t *, int) {
      if (on_smoothed) on_smoothed(utime, slot);
    });
  }
  // The same pass for a batch of INDEPENDENT log segments (SegmentBatcher): a filter need not have an INS update at every step.  Step j
  // runs pb_smooth_step_masked with the mask of INS update j+1 (RBISIMUProcessStep::stepMask): a filter without a message there keeps
  // the smoothed posterior of step j+1, which is its smoothed posterior at its own step (pronto_batch.h).  A step whose mask has no zero
  // -- known on the host for masks that came from the host, may_idle -- runs plain pb_smooth_step, with no select launch; with no mask in
  // the window the smoothed posteriors are bit for bit those of the two-argument pass.  smoother_masked_steps counts the select launches.
  // terminal_slot >= 0 (a slot taken out of the pool with reserveSlot): "next" of the newest step instead of the head -- every filter's
  // posterior at the end of ITS log, where the head of a filter whose segment ended early is not (its idle steps re-derive its angular
  // velocity / acceleration entries).  on_smoothed(utime of INS_j, slot, valid, valid_mem): valid = INS update j's mask, NULL when it has
  // none; valid_mem = where it lives (stepMask): PB_HOST for a step built from host messages, PB_DEVICE for one built on the device.
  int EKFSmoothBackwardsPass(double dt, int terminal_slot,
                             const std::function<void(int64_t utime, int slot, const uint8_t *valid, int valid_mem)> &on_smoothed)
  {
    if (terminal_slot >= history_slots || (terminal_slot >= 0 && std::find(free_slots.begin(), free_slots.end(), terminal_slot) != free_slots.end())) {
      fprintf(stderr, "EKFSmoothBackwardsPass: terminal slot %d is not a slot taken with reserveSlot()\n", terminal_slot);
      return -1;
    }
    return smooth_pass(dt, terminal_slot, true, on_smoothed);
  }
  // a checkpoint slot taken out of the pool for the caller (the history never recycles it); -1 = none is free.  releaseSlot gives it back.
  int reserveSlot()
  {
    if (free_slots.empty()) return -1;
    const int slot = free_slots.back();
    free_slots.pop_back();
    return slot;
  }
  void releaseSlot(int slot)
  {
    if (slot >= 0 && slot < history_slots && std::find(free_slots.begin(), free_slots.end(), slot) == free_slots.end()) free_slots.push_back(slot);
  }

private:
  int smooth_pass(double dt, int terminal_slot, bool masked, const std::function<void(int64_t, int, const uint8_t *, int)> &on_smoothed)
  {
    auto &map = history.updateMap;
    flushPending();
    // time-ordered list of (update, slot or -1)
    std::vector<std::pair<RBISUpdateInterface *, int>> seq;
    for (auto u = map.begin(); u != unprocessed_updates_start; ++u) seq.push_back({ u->second, slot_of(u->second) });
    const int N = (int) seq.size();
    if (N == 0 || seq[0].second < 0) {
      fprintf(stderr, "EKFSmoothBackwardsPass: the oldest update of the history has no checkpoint (state_estimator.history_slots = 0?)\n");
      return -1;
    }
    std::vector<int> ins, cks;
    for (int i = 0; i < N; i++) {
      if (seq[(size_t) i].first->sensor_id == RBISUpdateInterface::ins) ins.push_back(i);
      if (seq[(size_t) i].second >= 0) cks.push_back(i);
    }
    if (ins.size() < 2) return 0;
    // the longest run of updates without a checkpoint decides the window
    int maxgap = N - 1 - cks.back();
    for (size_t m = 0; m + 1 < cks.size(); m++) maxgap = std::max(maxgap, cks[m + 1] - cks[m] - 1);
    const bool head_loose = seq.back().second < 0;   // the newest posterior exists only as the device head
    const bool pair_out = fuse_ins_legodo && maxgap > 0;   // a re-applied pair whose partner has a checkpoint writes one slot further
    const int need = maxgap + 2 + ((maxgap > 0 || head_loose) ? 1 : 0) + (pair_out ? 1 : 0);
    if ((int) free_slots.size() < need) {
      fprintf(stderr, "EKFSmoothBackwardsPass: needs %d free checkpoint slots (two for the smoothed posteriors%s%s), %zu are free: raise "
                      "state_estimator.history_slots or lower history_checkpoint_every\n",
              need, maxgap > 0 ? ", the longest run of updates without a checkpoint and one for the head" : (head_loose ? ", one for the head" : ""),
              pair_out ? ", one for the posterior of a re-applied fused pair" : "", free_slots.size());
      return -1;
    }
    const size_t nf = free_slots.size();
    const int spare[2] = { free_slots[nf - 1], free_slots[nf - 2] };
    const int head_keep = (maxgap > 0 || head_loose) ? free_slots[nf - 3] : -1;
    auto W = [&](int i) { return free_slots[nf - 4 - (size_t) i]; };   // window slots
    int rc = PB_OK;
    bool head_saved = false;
    // an error leaves no output / predicted slot pending and the newest posterior as the head (re-applied updates may have moved it)
    auto bail = [&](const char *what) {
      last_status = rc;
      fprintf(stderr, "EKFSmoothBackwardsPass: %s: %s\n", what, pb_last_error(ctx));
      pb_set_pred_slot(ctx, -1);
      pb_set_output_slot(ctx, -1);
      if (head_saved && pb_state_restore(ctx, head_keep) == PB_OK) pb_set_utime(ctx, head_utime);
      device_head = nullptr;
      return -1;
    };
    if (head_keep >= 0) {
      if (device_head != seq.back().first) {
        fprintf(stderr, "EKFSmoothBackwardsPass: the device does not hold the newest posterior (call it right after addUpdate)\n");
        return -1;
      }
      if ((rc = pb_state_save(ctx, head_keep)) != PB_OK) return bail("saving the head");
      head_saved = true;
    }
    int next = terminal_slot >= 0 ? terminal_slot : (head_loose ? head_keep : seq.back().second), steps = 0, toggle = 0;
    int j = (int) ins.size() - 2;   // the step being smoothed: needs the posteriors of updates ins[j+1] - 1 and ins[j+1]
    // stretches (a, e]: a = a checkpointed update, e = the next checkpointed update (or the newest update)
    for (int m = (int) cks.size() - 1; m >= 0 && j >= 0; m--) {
      const int a = cks[(size_t) m], e = (m + 1 < (int) cks.size()) ? cks[(size_t) m + 1] : N - 1;
      if (ins[(size_t) j + 1] <= a) continue;          // (no INS update in this stretch)
      const int last_missing = (seq[(size_t) e].second >= 0) ? e - 1 : e;
      if (last_missing > a) {                          // re-derive the posteriors of a+1 .. last_missing into the window
        if ((rc = pb_state_restore(ctx, seq[(size_t) a].second)) != PB_OK) return bail("restoring a checkpoint");
        for (int i = a + 1; i <= last_missing; i++) {
          auto *imu = as_imu(seq[(size_t) i].first);
          if (imu != nullptr && imu->ran_fused && i + 1 <= e) {   // the pair: prediction -> W(i - a - 1), posterior -> W(i - a)
            const PairPlan pair = plan_pair(imu, seq[(size_t) i + 1].first);
            pb_set_output_slot(ctx, W(i - a));
            if ((rc = pb_set_pred_slot(ctx, W(i - a - 1))) != PB_OK) return bail("setting the predicted slot");
            if (pair) {
              if ((rc = run_fused(imu, pair)) != PB_OK) return bail("re-applying a fused pair");
              smoother_reapplied_updates += 2;
              smoother_reapplied_pairs++;
              i++;
              continue;
            }
            // no fused re-application of this partner (a six-row leg-odometry measurement whose pair kernel has run): the two
            // halves one after the other -- the prediction exactly, the partner's posterior to rounding of the pair kernel's
            pb_set_pred_slot(ctx, -1);
            pb_set_output_slot(ctx, -1);
          }
          pb_set_output_slot(ctx, W(i - a - 1));
          if ((rc = seq[(size_t) i].first->updateFilter(ctx)) != PB_OK) return bail("re-applying an update");
          smoother_reapplied_updates++;
        }
      }
      auto slot_at = [&](int i) { return seq[(size_t) i].second >= 0 ? seq[(size_t) i].second : W(i - a - 1); };
      while (j >= 0 && ins[(size_t) j + 1] > a) {
        const int ip = ins[(size_t) j + 1];
        const int out = spare[toggle];
        int step_mem = PB_DEVICE;
        const uint8_t *step = nullptr;
        if (masked)
          if (const auto *nx = as_imu(seq[(size_t) ip].first))
            if (nx->may_idle) step = nx->stepMask(step_mem);
        if (step != nullptr) {
          if ((rc = pb_smooth_step_masked(ctx, slot_at(ip), next, slot_at(ip - 1), out, dt, step, step_mem)) != PB_OK) return bail("smoother step");
          smoother_masked_steps++;
        } else if ((rc = pb_smooth_step(ctx, slot_at(ip), next, slot_at(ip - 1), out, dt)) != PB_OK) {
          return bail("smoother step");
        }
        if (on_smoothed) {
          int cur_mem = PB_DEVICE;
          const auto *cu = as_imu(seq[(size_t) ins[(size_t) j]].first);
          const uint8_t *cur_valid = cu != nullptr ? cu->stepMask(cur_mem) : nullptr;
          on_smoothed(seq[(size_t) ins[(size_t) j]].first->utime, out, cur_valid, cur_mem);
        }
        next = out;
        toggle ^= 1;
        steps++;
        j--;
      }
    }
    if (head_keep >= 0) {
      if ((rc = pb_state_restore(ctx, head_keep)) != PB_OK) return bail("putting the head back");   // the newest posterior again
      pb_set_utime(ctx, head_utime);
    }
    device_head = nullptr;  // callers may have restored slots into the head: force a restore on the next replay
    return steps;
  }

  bool flushing_ = false;
  int holding_ = 0;  // updates at the end of the history that have not been applied yet (0, 1 = an INS step, 2 = INS + legodo)
  static RBISIMUProcessStep *as_imu(RBISUpdateInterface *u) { return dynamic_cast<RBISIMUProcessStep *>(u); }
  // the measurement object that carries a deferred leg odometry (pair_kernel / make_measurement): the update itself, or the
  // six-row half of LegOdoCommon's pos_and_lin_rate either-update (its block holds both halves' rows and masks)
  static RBISIndexedMeasurement *deferredMeasurement(RBISUpdateInterface *u)
  {
    if (auto *e = dynamic_cast<RBISEitherUpdate *>(u)) u = e->first;
    return dynamic_cast<RBISIndexedMeasurement *>(u);
  }
  // How an INS step and the update behind it run as ONE launch (fuse_ins_legodo), if they can.  plan_pair is the only place that decides
  // it; whoever holds a plan other than `none` -- the roll-forward loop, which reserves the pair's checkpoint slot on its word, and
  // EKFSmoothBackwardsPass -- hands it to run_fused, which executes it and cannot decline.
  struct PairPlan {
    enum Kind {
      none,          // not fusible: the two updates run one after the other
      pair_kernel,   // the measurement is made inside the step kernel (leg odometry, any of LegOdoCommon's modes)
      device_block,  // IMU block from the host (broadcast or per filter), measurement one [6][B] block on the device
      broadcast,     // one robot's IMU message and measurement for every filter
      host_blocks    // per-filter host blocks, R diagonal: per filter or broadcast
    } kind = none;
    RBISIndexedMeasurement *m = nullptr;   // the measurement (pair_kernel: the one that carries the kernel, deferredMeasurement)
    explicit operator bool() const { return kind != none; }
  };
  PairPlan plan_pair(const RBISIMUProcessStep *imu, RBISUpdateInterface *next) const
  {
    if (auto *d = deferredMeasurement(next))
      if (d->pair_kernel) return { PairPlan::pair_kernel, d };
    if (dynamic_cast<RBISIndexedPlusOrientationMeasurement *>(next) != nullptr) return {};
    auto *m = dynamic_cast<RBISIndexedMeasurement *>(next);
    if (m == nullptr || m->index != RBIS::velocityInds()) return {};
    if (device_lo_block(m)) return { PairPlan::device_block, m };
    if (imu->imu_block.mem == PB_HOST_BROADCAST && m->measurement.mem == PB_HOST_BROADCAST && m->r_kind == PB_R_DIAG_BROADCAST && m->mask == nullptr)
      return { PairPlan::broadcast, m };
    if (imu->imu_block.mem == PB_HOST && m->measurement.mem == PB_HOST && m->cov_mem == PB_HOST && (m->r_kind == PB_R_DIAG || m->r_kind == PB_R_DIAG_BROADCAST))
      return { PairPlan::host_blocks, m };
    return {};
  }
  // an INS step followed by the velocity measurement LegOdoCommon's lin_rate mode produces, or by a measurement with a pair kernel
  bool fusible_pair(const RBISIMUProcessStep *imu, RBISUpdateInterface *next) const { return (bool) plan_pair(imu, next); }
  // a velocity measurement that lives on the device as ONE [6][B] block (z, diagonal R) + mask: what
  // LegOdoHandler::processMessageFeet / pb_legodo_update(_after_predict) leave there
  bool device_lo_block(const RBISIndexedMeasurement *m) const
  {
    return m->measurement.mem == PB_DEVICE && m->r_kind == PB_R_DIAG && m->measurement_cov == m->measurement.p + (size_t) 3 * B;
  }
  // the [6][B] host block of a host_blocks pair (z, then the diagonal of R: per filter, or one robot's broadcast), in fuse_lo_
  const double *host_lo_block(const RBISIndexedMeasurement *m)
  {
    fuse_lo_.resize((size_t) 6 * B);
    memcpy(fuse_lo_.data(), m->measurement.p, sizeof(double) * 3 * B);
    if (m->r_kind == PB_R_DIAG) memcpy(fuse_lo_.data() + (size_t) 3 * B, m->measurement_cov, sizeof(double) * 3 * B);
    else
      for (int i = 0; i < 3; i++) std::fill_n(fuse_lo_.begin() + (size_t) (3 + i) * B, B, m->measurement_cov[i]);
    return fuse_lo_.data();
  }
  std::vector<double> fuse_lo_;
  // executes a planned pair (pair.kind != none) as one launch -- pb_step_legodo, _split or the pair kernel -- and returns its pb_status
  int run_fused(RBISIMUProcessStep *imu, const PairPlan &pair)
  {
    RBISIndexedMeasurement *m = pair.m;
    if (pair.kind == PairPlan::pair_kernel) {  // one launch for the message pair
      const int rc = m->pair_kernel(ctx, imu, history_slots > 0);
      m->pair_kernel = nullptr;
      m->make_measurement = nullptr;
      leg_kernel_pairs++;
      return rc;
    }
    const double q[4] = { imu->q_gyro, imu->q_accel, imu->q_gyro_bias, imu->q_accel_bias };
    imu->announce(ctx);   // (taken by whichever step call follows)
    if (pair.kind == PairPlan::device_block) return pb_step_legodo_split(ctx, imu->imu_block.p, imu->imu_block.mem, m->measurement.p, m->mask, PB_DEVICE, q);
    if (pair.kind == PairPlan::broadcast) {
      const double lo[6] = { m->measurement.p[0], m->measurement.p[1], m->measurement.p[2],
                             m->measurement_cov[0], m->measurement_cov[1], m->measurement_cov[2] };
      return pb_step_legodo(ctx, imu->imu_block.p, lo, nullptr, q, PB_HOST_BROADCAST);
    }
    return pb_step_legodo(ctx, imu->imu_block.p, host_lo_block(m), m->mask, q, PB_HOST);
  }
  // a broadcast or host_blocks pair followed by a position_orient / position_yaw correction with a diagonal R -> one
  // pb_step_legodo_correct; false = these three do not run as one (nothing has run then)
  bool run_fused3(RBISIMUProcessStep *imu, const PairPlan &pair, RBISUpdateInterface *third, int &rc)
  {
    // (a device-resident leg-odometry block, or one still to be made by a pair kernel, pairs: it does not triple)
    if (pair.kind != PairPlan::broadcast && pair.kind != PairPlan::host_blocks) return false;
    auto *o = dynamic_cast<RBISIndexedPlusOrientationMeasurement *>(third);
    if (o == nullptr) return false;
    int kind;
    if (o->index == std::vector<int>{ 9, 10, 11, 6, 7, 8 }) kind = PB_CORR_POS_ORIENT;
    else if (o->index == std::vector<int>{ 9, 10, 11, 8 }) kind = PB_CORR_POS_YAW;
    else return false;
    if (o->r_kind != PB_R_DIAG && o->r_kind != PB_R_DIAG_BROADCAST) return false;
    if (o->measurement.mem != o->orientation.mem) return false;
    if (o->r_kind == PB_R_DIAG && o->cov_mem != o->measurement.mem) return false;
    const RBISIndexedMeasurement *m = pair.m;
    const double q[4] = { imu->q_gyro, imu->q_accel, imu->q_gyro_bias, imu->q_accel_bias };
    const bool bcast = pair.kind == PairPlan::broadcast;
    double lo6[6];
    if (bcast)
      for (int i = 0; i < 3; i++) { lo6[i] = m->measurement.p[i]; lo6[3 + i] = m->measurement_cov[i]; }
    const double *lo = bcast ? lo6 : host_lo_block(m);
    imu->announce(ctx);
    rc = pb_step_legodo_correct(ctx, imu->imu_block.p, lo, bcast ? nullptr : m->mask, q, bcast ? PB_HOST_BROADCAST : PB_HOST, kind, o->measurement.p,
                                o->measurement_cov, o->r_kind, o->orientation.p, o->mask, o->measurement.mem);
    return true;
  }
  // One step of the roll-forward: update u on its own, or -- given the INS step in front of it and their plan -- the two as one fused
  // launch, which counts 2 towards the checkpoint cadence.  When the cadence gives the step a checkpoint, the posterior is written
  // straight into the slot (no copy afterwards) and recorded for u: a pair is checkpointed behind its SECOND half, so that a replay
  // which starts there continues behind the pair.
  void apply_step(RBISUpdateInterface *u, RBISIMUProcessStep *paired_imu, const PairPlan &pair)
  {
    // (a pair that reserves a slot here cannot be declined afterwards: run_fused executes the plan the caller classified it with, so
    // the slot always ends up in checkpoint_of and no output slot stays pending)
    int slot = -1;
    if (history_slots > 0 && (since_checkpoint += paired_imu ? 2 : 1) >= checkpoint_every && (slot = reserve_slot(u)) >= 0)
      pb_set_output_slot(ctx, slot);
    int rc;
    if (paired_imu != nullptr) {
      rc = run_fused(paired_imu, pair);
      paired_imu->ran_fused = true;
      fused_pairs++;
    } else {
      if (auto *imu = as_imu(u)) imu->ran_fused = false;
      rc = u->updateFilter(ctx);
    }
    if (rc != PB_OK) {
      last_status = rc;
      if (paired_imu != nullptr) fprintf(stderr, "MavStateEstimator::addUpdate: fused ins+legodo step failed: %s\n", pb_last_error(ctx));
      else
        fprintf(stderr, "MavStateEstimator::addUpdate: %s update failed: %s\n", RBISUpdateInterface::sensor_enum_string(u->sensor_id), pb_last_error(ctx));
    }
    device_head = u;
    head_utime = u->utime;  // posterior_state.utime = update->utime (:60)
    if (slot >= 0) {
      pb_set_output_slot(ctx, -1);
      rc = pb_state_save(ctx, slot);  // a no-op when the step wrote there; a copy for updates that cannot (reset)
      if (rc != PB_OK) last_status = rc;
      checkpoint_of[u] = slot;
      since_checkpoint = 0;
    }
  }
  // the checkpoint slot that holds u's posterior, -1 = none
  int slot_of(RBISUpdateInterface *u) const
  {
    auto it = checkpoint_of.find(u);
    return it == checkpoint_of.end() ? -1 : it->second;
  }
  // the newest element at or before `it` that has a checkpoint (begin() always has one)
  updateHistory::historyMapIterator checkpoint_at_or_before(updateHistory::historyMapIterator it) const
  {
    while (slot_of(it->second) < 0) --it;
    return it;
  }
  void drop_checkpoint(RBISUpdateInterface *u)
  {
    auto it = checkpoint_of.find(u);
    if (it != checkpoint_of.end()) {
      free_slots.push_back(it->second);
      checkpoint_of.erase(it);
    }
  }
  // a free checkpoint slot for update u, recycling the oldest part of the window when the pool is exhausted; -1 = none
  int reserve_slot(RBISUpdateInterface *u)
  {
    if (free_slots.empty()) {
      // pool exhausted: the window shrinks to what the pool covers -- drop everything before the second-oldest
      // checkpoint (begin() must keep one: it is the prior of the oldest replayable update)
      auto &map = history.updateMap;
      auto it = map.begin();
      ++it;
      while (it != map.end() && slot_of(it->second) < 0) ++it;
      if (it == map.end() || it->second == u) return -1;  // nothing to recycle: skip this checkpoint
      erase_before(it);
    }
    const int slot = free_slots.back();
    free_slots.pop_back();
    return slot;
  }
  void save_checkpoint(RBISUpdateInterface *u)
  {
    const int slot = reserve_slot(u);
    if (slot < 0) return;
    int rc = pb_state_save(ctx, slot);
    if (rc != PB_OK) last_status = rc;
    checkpoint_of[u] = slot;
    since_checkpoint = 0;
  }
  void erase_before(updateHistory::historyMapIterator keep)
  {
    auto &map = history.updateMap;
    for (auto it = map.begin(); it != keep; ++it) {
      drop_checkpoint(it->second);
      delete it->second;
    }
    map.erase(map.begin(), keep);
  }
  // update_history.cpp:44-55, with the extra rule that the new first element must hold a checkpoint
  void clearHistoryBeforeUtime(int64_t utime)
  {
    auto &map = history.updateMap;
    if (history_slots == 0) {  // in-order only: keep just the head
      auto last = map.end();
      --last;
      for (int h = 0; h < holding_; h++) --last;  // held-back updates have not been applied: the head is before them
      erase_before(last);
      return;
    }
    auto keep = map.begin();
    for (auto it = map.begin(); it != map.end() && it->first <= utime; ++it)
      if (slot_of(it->second) >= 0) keep = it;
    if (keep != map.begin()) erase_before(keep);
  }
};

}  // namespace MavStateEst
