// mav_state_est_batch.hpp -- host-side C++ mirror of Pronto's plugin / update-object API for B filters at once,
// header-only on top of the C ABI (include/pronto_batch.h).  Same namespace, class and method names, argument
// meaning and error conventions as the reference for THIS path, so handler code reads like the reference's:
//
//   RBISUpdateInterface + RBISResetUpdate / RBISIMUProcessStep / RBISIndexedMeasurement /
//   RBISIndexedPlusOrientationMeasurement          state-estimator/src/mav_state_est/rbis_update_interface.hpp:8-120
//   MavStateEstimator::addUpdate / getHeadState / getMeasurementsLogLikelihood   mav_state_est.hpp:10-25, .cpp:28-96
//       (these, BotParam, RBIS / RBIM and updateHistory are in mav_state_est.hpp, included first below)
//   InsHandler, ScanMatcherHandler, IndexedMeasurementHandler, GpsHandler        sensor_handlers.hpp:22-167
//   LegOdoCommon (+ a LegOdoHandler fed by leg-odometry deltas)                  mav_est_legodo/rbis_legodo_common.hpp
//   FovisHandler                                                                 mav_est_fovis/rbis_fovis_update.cpp:6-312
//   SensorHandler<Msg,Handler> dispatch (downsample gate, utime_offset, roll_forward)   lcm_front_end.hpp:139-203
//
// What changes, and why: every message type carries B filters' worth of data (SoA, filter index fastest, host or
// device memory); RBIS/RBIM are batched host containers; updateFilter() applies itself to the estimator's
// device-resident posterior instead of taking prior/posterior by value (the posterior of 65 536 filters is 73 MB --
// it stays in HBM).  BotParam is a key/value map with the reference's key names; *_or_fail keep libbot's behaviour
// (message on stderr, exit(1)).  LCM, BotFrames and the leg kinematics are outside this path.
//
// Throughput note: a handler that transforms inputs on the host (frame rotation in InsHandler, delta->velocity in
// LegOdoCommon) costs O(B) host work per message; bulk replays pre-stage body-frame blocks in HBM and use
// pb_run_legodo (see bench.py).  The handlers skip the host pass entirely when the transform is the identity.
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

#include "mav_state_est.hpp"  // BotParam, RBIS / RBIM, the update objects, updateHistory, MavStateEstimator
#include "lcm_schema.hpp"  // includes pronto_wire.hpp

// The handlers' per-filter host loops (frame rotation, velocity from deltas ...) are independent per filter: compile the
// host program with -fopenmp and they run on all cores; without it the pragma disappears.
#ifdef _OPENMP
#include <omp.h>
// At most PRONTO_SHIM_THREADS host threads (default 16: the CPU share a one-GPU job gets on a shared box, whatever the machine's
// core count says -- a team of 128 spinning threads on a 16-CPU quota is slower than one thread by orders of magnitude).
static inline int pb_shim_threads()
{
  static const int n = [] {
    const char *e = getenv("PRONTO_SHIM_THREADS");
    const int want = e ? atoi(e) : 16;
    return std::max(1, std::min(want, omp_get_max_threads()));
  }();
  return n;
}
#define PB_SHIM_PARALLEL_FOR _Pragma("omp parallel for schedule(static) num_threads(pb_shim_threads())")
#define PB_SHIM_PRAGMA(x) _Pragma(#x)
#define PB_SHIM_PARALLEL_FOR_SUM(v) PB_SHIM_PRAGMA(omp parallel for schedule(static) num_threads(pb_shim_threads()) reduction(+ : v))
#else
#define PB_SHIM_PARALLEL_FOR
#define PB_SHIM_PARALLEL_FOR_SUM(v)
#endif

namespace MavStateEst {

// ---------------------------------------------------------------------------------------------------------------
// messages (batched stand-ins for the LCM types at the seam; every array is [k][B])
// ---------------------------------------------------------------------------------------------------------------
namespace msgs {
struct ins_t {               // bot_core::ins_t
  int64_t utime;
  BatchArray gyro, accel;    // [3][B] each, sensor frame
  BatchArray mag;            // [3][B] magnetometer, sensor frame; optional (p == NULL: zeros, like the Atlas path :274)
  const uint8_t *valid = nullptr;  // [B], in the memory space of gyro / accel (independent log segments, SegmentBatcher /
                                   // SegmentStreamer): 0 = this filter has no message -- its segment has ended -- and idles: its
                                   // step is taken with dt = 0
};
struct kvh_raw_imu_t {       // the newest packet of bot_core::kvh_raw_imu_batch_t (atlas_filter == false path)
  int64_t utime;
  BatchArray delta_rotation, linear_acceleration;  // [3][B]
  double raw_dt;             // (raw_imu[0].utime - raw_imu[1].utime) * 1E-6
};
struct legodo_delta_t {      // what leg_estimate hands to LegOdoCommon::createMeasurement
  int64_t utime, prev_utime;
  const double *position;        // [3][B] pelvis position (may be NULL unless mode pos_and_lin_rate), host
  const double *delta_trans;     // [3][B] translation of the pelvis delta over (prev_utime, utime], host
  const double *delta_quat;      // [4][B] rotation of the delta (NULL = identity), host
  const int *position_status;    // [B] or NULL (= valid)
  const float *delta_status;     // [B]: < 0 skip (leg_estimate.hpp:84-93), < 0.5 certain, else uncertain
};
struct foot_state_t {        // what forward kinematics + the foot sensors give per joint-state message (leg_estimate.cpp:430-447)
  int64_t utime;
  BatchArray feet;           // [14][B]: body-to-left-foot (t3, q4 = w,x,y,z), body-to-right-foot (t3, q4)
  BatchArray forces;         // [2][B]: left, right vertical foot force
};
struct joint_state_t {       // bot_core::joint_state_t: the arrays are float on the wire and here
  int64_t utime;
  std::vector<std::string> joint_name;      // num_joints names, the same for every filter
  const float *joint_position = nullptr;    // [num_joints][B] (PB_HOST / PB_DEVICE) or [num_joints] (PB_HOST_BROADCAST)
  const float *joint_velocity = nullptr;    // (only the joint Kalman filter reads it, leg_estimate.cpp:418-426)
  const float *joint_effort = nullptr;      // same shape as joint_position; read when legodo.torque_adjustment is set
  int mem = PB_HOST;                        // PB_DEVICE arrays must stay valid until the next message (see LegOdoHandler::forceTorqueDevice)
  // independent log segments (one recorded robot per filter, SegmentBatcher): every filter's message has its OWN time stamp
  // -- utimes [B], HOST; `utime` above then is the batch-level time that orders the update in the history -- and a filter whose
  // segment has ended has no message at all: valid [B], HOST, 0 = none.  NULL = one time for all / all valid.
  const int64_t *utimes = nullptr;
  const uint8_t *valid = nullptr;
  int times_mem = PB_HOST;                  // where utimes / valid live: PB_HOST, or PB_DEVICE (chunked replays: read in place)
};
struct six_axis_force_torque_array_t {   // bot_core::six_axis_force_torque_array_t: what the leg odometry reads of it
  int64_t utime;
  BatchArray force_z;        // [2][B] (PB_HOST) or [2] (PB_HOST_BROADCAST): sensors[0].force[2], sensors[1].force[2] (left, right foot)
};
struct controller_foot_contact_t {       // pronto::controller_foot_contact_t
  int64_t utime;
  int32_t num_left_foot_contacts, num_right_foot_contacts;
};
struct controller_status_t {   // pronto::controller_status_t (pronto_controller_status_t.lcm)
  enum { UNKNOWN = 0, STANDING = 1, WALKING = 2, HARNESSED = 3, QUASISTATIC = 4, BRACING = 5, CRAWLING = 6, DUMMY = 7, MANIPULATING = 8 };
  int64_t utime = 0;
  int8_t state = UNKNOWN;
  int64_t controller_utime = 0;
  float V = 0, Vdot = 0;
};
struct behavior_t {            // pronto::behavior_t (pronto_behavior_t.lcm)
  enum { BEHAVIOR_NONE = 0, BEHAVIOR_FREEZE = 1, BEHAVIOR_STAND_PREP = 2, BEHAVIOR_STAND = 3, BEHAVIOR_WALK = 4, BEHAVIOR_STEP = 5,
         BEHAVIOR_MANIPULATE = 6, BEHAVIOR_USER = 7, BEHAVIOR_CALIBRATE = 8, BEHAVIOR_SOFT_STOP = 9 };
  int64_t utime = 0;
  int32_t behavior = BEHAVIOR_NONE;
};
struct update_t {            // pronto::update_t (fovis)
  int64_t timestamp, prev_timestamp;
  const uint8_t *estimate_valid;   // [B] or NULL: estimate_status == ESTIMATE_VALID
  BatchArray translation, rotation;  // [3][B], [4][B]
};
struct pose_t {              // bot_core::pose_t
  int64_t utime;
  BatchArray pos, vel, orientation;  // [3][B], [3][B], [4][B]
  const uint8_t *valid = nullptr;    // [B] HOST, PB_HOST messages only: 0 = this filter has no message (independent log segments)
};
struct indexed_measurement_t {  // pronto::indexed_measurement_t
  int64_t utime;
  std::vector<int> z_indices;
  BatchArray z_effective;      // [m][B]
  const double *R_effective;   // [m*m][B] column-major, same memory space as z_effective
};
struct rigid_transform_t {  // bot_core::rigid_transform_t (Vicon)
  int64_t utime;
  BatchArray trans, quat;    // [3][B], [4][B] host (or host-broadcast) arrays
};
struct gps_data_t {
  int64_t utime;
  const uint8_t *has_lock;     // [B]: gps_lock >= 3
  BatchArray xyz_pos;
};
struct kvh_raw_imu_packet_t {  // bot_core::kvh_raw_imu_t
  int64_t utime, packet_count;
  const double *delta_rotation, *linear_acceleration;  // [3][B] host arrays
};
struct kvh_raw_imu_batch_t {   // bot_core::kvh_raw_imu_batch_t: raw_imu[0] is the NEWEST packet, as on the wire
  int64_t utime;
  std::vector<kvh_raw_imu_packet_t> raw_imu;
  int mem = PB_HOST;           // PB_HOST_BROADCAST: the packets' arrays are [3], one robot's IMU for every filter
};
// B DIFFERENT robots' kvh_raw_imu_batch_t messages as one batched message (independent log segments): every robot's message has
// been through ITS OWN IMUStream::convertFromLCMBatch (imu_stream.cpp:62-98) where it was decoded, and what is left of it is
// what InsHandler::processMessageAtlas reads (sensor_handlers.cpp:173-204).  All arrays live in `mem` (PB_HOST or PB_DEVICE).
struct kvh_raw_imu_segments_t {
  int64_t utime;                 // batch-level time (orders the update in the history)
  int max_new = 0;               // rows of new_accel: the most new packets any filter can have in one message
  const int32_t *n_new = nullptr;         // [B] new packets of filter b; 0 = "no new IMU packets": no update for it (:181-187)
  const uint8_t *valid = nullptr;         // [B] n_new[b] > 0 and the filter has a message at all
  const double *new_accel = nullptr;      // [max_new][3][B] linear_acceleration of the new packets, oldest first
  const double *delta_rotation = nullptr; // [3][B] of the newest new packet
  const double *raw_dt = nullptr;         // [B] that packet's utime_delta * 1E-6 (atlas_filter), or (raw_imu[0].utime - raw_imu[1].utime) * 1E-6
  const int64_t *utimes = nullptr;        // [B] every robot's own message utime
  int mem = PB_HOST;
};
}  // namespace msgs

// estimate_tools/src/estimate_tools/imu_stream.hpp:10-37, imu_stream.cpp:62-98: KVH batch messages repeat packets
// (1 kHz packets in ~333 Hz batches); only packets with a packet_count above the last one seen are new.
struct IMUPacket {
  int64_t utime_raw, utime_batch, utime, utime_delta, packet_count;
  const double *delta_rotation, *linear_acceleration;  // [3][B]
};
struct IMUBatch {
  int64_t utime;
  std::vector<IMUPacket> packets;      // new packets, [0] oldest ... [end] newest
  std::vector<IMUPacket> packets_old;  // packets already seen in an earlier message
};
// estimate_tools/src/estimate_tools/iir_notch.cpp:3-61: 2nd-order IIR notch, host version.  The batch runs the cascade
// on the device (pb_imu_notch, one state per filter); when ONE robot's IMU feeds every filter (PB_HOST_BROADCAST) every
// filter would compute the same numbers, so the handler filters once on the host -- the reference's own code path.
class IIRNotch {
public:
  double b[3], a[3], x[2] = { 0, 0 }, y[2] = { 0, 0 };
  IIRNotch(double notch_freq, double fs)
  {
    const double Wo0 = notch_freq / (fs / 2), Ab = fabs(10 * log10(.5));
    const double BW = Wo0 * M_PI, Wo = Wo0 * M_PI;      // "Inputs are normalized by pi" (:21-23); Bw = Wo (:8)
    const double Gb = pow(10, -Ab / 20.);
    const double beta = (sqrt(1.0 - Gb * Gb) / Gb) * tan(BW / 2.0);
    const double gain = 1 / (1 + beta);
    b[0] = gain; b[1] = gain * (-2.0 * cos(Wo)); b[2] = gain;
    a[0] = 1.0; a[1] = -2 * gain * cos(Wo); a[2] = 2 * gain - 1;
  }
  double processSample(double input)
  {
    const double output = (input * b[0] + x[0] * b[1] + x[1] * b[2]) - (y[0] * a[1] + y[1] * a[2]);  // :52
    x[1] = x[0]; x[0] = input;
    y[1] = y[0]; y[0] = output;
    return output;
  }
};

// The de-duplication rule of imu_stream.cpp:62-98 on plain numbers, one state per packet stream: IMUStream below uses it for one
// robot's messages, the segment replayers' KVH decoder (segment_channels.hpp) keeps one per log segment.
struct IMUStreamRule {
  int64_t last_packet = -1, last_packet_utime = 0;
  // in front of a message's packets: a newest packet count that went backwards is a time skip and resets the stream (:63-68)
  bool resetIfBackwards(int64_t newest_packet_count)
  {
    if (newest_packet_count >= last_packet) return false;
    last_packet = -1;
    last_packet_utime = 0;
    return true;
  }
  // per packet, oldest first: true = new (a packet count above the last one seen), with its time behind the last accepted packet's
  bool accept(int64_t packet_count, int64_t utime, int64_t &utime_delta)
  {
    if (packet_count <= last_packet) return false;
    utime_delta = utime - last_packet_utime;
    last_packet = packet_count;
    last_packet_utime = utime;
    return true;
  }
};

class IMUStream {
public:
  IMUBatch convertFromLCMBatch(const msgs::kvh_raw_imu_batch_t *msg)
  {
    if (!msg->raw_imu.empty() && rule_.resetIfBackwards(msg->raw_imu[0].packet_count)) {
      fprintf(stdout, "Detected time skip, resetting IMUStream\n");  // imu_stream.cpp:63-68
      counter_ = 0;
    }
    IMUBatch batch;
    batch.utime = msg->utime;
    for (int i = (int) msg->raw_imu.size() - 1; i >= 0; i--) {  // oldest first (:76)
      const auto &m = msg->raw_imu[i];
      IMUPacket raw;
      raw.utime_raw = m.utime;
      raw.utime_batch = msg->utime;
      raw.utime = m.utime;
      raw.packet_count = m.packet_count;
      raw.delta_rotation = m.delta_rotation;
      raw.linear_acceleration = m.linear_acceleration;
      if (rule_.accept(m.packet_count, m.utime, raw.utime_delta)) {
        batch.packets.push_back(raw);
      } else {
        raw.utime_delta = m.utime - (-m.utime);  // "deliberately obfuscate the delta field" (:87-88)
        batch.packets_old.push_back(raw);
      }
    }
    counter_++;
    return batch;
  }
  int getNumberBatchSinceReset() const { return counter_; }

private:
  IMUStreamRule rule_;
  int counter_ = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// handlers
// ---------------------------------------------------------------------------------------------------------------
// RBISInitializer's bookkeeping helpers (rbis_initializer.cpp:96-113)
struct RBISInitializer {
  static bool allInitializedExcept(const std::map<std::string, bool> &sensors_initialized, const std::string &sensor_prefix)
  {
    for (const auto &kv : sensors_initialized) {
      if (kv.first == sensor_prefix) continue;
      if (!kv.second) return false;
    }
    return true;
  }
  static bool initializingWith(const std::map<std::string, bool> &sensors_initialized, const std::string &sensor_prefix)
  {
    return sensors_initialized.count(sensor_prefix) > 0;
  }
};

// Eigen's Quaternion::setFromTwoVectors(a, b) (w,x,y,z): the smallest rotation with q * a parallel to b; opposite
// vectors take any axis orthogonal to a (Eigen takes one from an SVD)
inline void quat_from_two_vectors(const double a[3], const double b[3], double q[4])
{
  const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  const double v0[3] = { a[0] / na, a[1] / na, a[2] / na }, v1[3] = { b[0] / nb, b[1] / nb, b[2] / nb };
  double c = v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2];
  if (c < -1.0 + 1e-12) {
    const int k = (fabs(v0[0]) < fabs(v0[1])) ? (fabs(v0[0]) < fabs(v0[2]) ? 0 : 2) : (fabs(v0[1]) < fabs(v0[2]) ? 1 : 2);
    double e[3] = { 0, 0, 0 };
    e[k] = 1.0;
    const double ax[3] = { v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0] };
    const double n = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (c < -1.0) c = -1.0;
    const double w2 = (1.0 + c) * 0.5;
    q[0] = sqrt(w2);
    for (int i = 0; i < 3; i++) q[1 + i] = ax[i] / n * sqrt(1.0 - w2);
    return;
  }
  const double axis[3] = { v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0] };
  const double sq = sqrt((1.0 + c) * 2.0), invs = 1.0 / sq;
  q[0] = sq * 0.5;
  for (int i = 0; i < 3; i++) q[1 + i] = axis[i] * invs;
}

class InsHandler {
public:
  std::string channel;
  BotTrans ins_to_body;
  double cov_accel, cov_gyro, cov_accel_bias, cov_gyro_bias, dt;
  bool atlas_filter, accel_bias_update_online, gyro_bias_update_online;
  int64_t prev_utime_atlas = 0;

  InsHandler(BotParam *_param, const BotTrans *ins_to_body_ = nullptr)
  {
    param_ = _param;
    channel = bot_param_get_str_or_fail(_param, "state_estimator.ins.channel");
    cov_gyro = bot_sq(bot_to_radians(bot_param_get_double_or_fail(_param, "state_estimator.ins.q_gyro")));          // :18-19
    cov_accel = bot_sq(bot_param_get_double_or_fail(_param, "state_estimator.ins.q_accel"));                        // :20-21
    cov_gyro_bias = bot_sq(bot_to_radians(bot_param_get_double_or_fail(_param, "state_estimator.ins.q_gyro_bias")));  // :22-23
    cov_accel_bias = bot_sq(bot_param_get_double_or_fail(_param, "state_estimator.ins.q_accel_bias"));              // :24-25
    dt = bot_param_get_double_or_fail(_param, "state_estimator.ins.timestep_dt");                                  // :27
    atlas_filter = bot_param_get_boolean_or_fail(_param, "state_estimator.ins.atlas_filter");
    accel_bias_update_online = bot_param_get_boolean_or_fail(_param, "state_estimator.ins.accel_bias_update_online");
    if (!accel_bias_update_online) cov_accel_bias = 0.0;                                                          // :70-72
    gyro_bias_update_online = bot_param_get_boolean_or_fail(_param, "state_estimator.ins.gyro_bias_update_online");
    if (!gyro_bias_update_online) cov_gyro_bias = 0.0;                                                            // :89-91
    if (ins_to_body_) ins_to_body = *ins_to_body_;
    notch_freq = atlas_filter ? bot_param_get_double_or_fail(_param, "state_estimator.ins.atlas_filter_freq") : 0.0;  // :31
  }

  // Atlas KVH path WITH the front end (sensor_handlers.cpp:173-197): de-duplicate the batch message, run every NEW
  // packet through the 3-stage notch cascade (on the device: pb_imu_notch), use the newest filtered packet.
  RBISUpdateInterface *processMessageAtlas(const msgs::kvh_raw_imu_batch_t *msg, MavStateEstimator *est)
  {
    const int B = est->B;
    if (msg->mem != PB_HOST && msg->mem != PB_HOST_BROADCAST) return nullptr;
    if (!atlas_filter) {
      // :199-204: newest packet unfiltered, raw_dt from the two newest packets
      if (msg->raw_imu.size() < 2) return nullptr;
      msgs::kvh_raw_imu_t m{ msg->utime, BatchArray(msg->raw_imu[0].delta_rotation, msg->mem),
                             BatchArray(msg->raw_imu[0].linear_acceleration, msg->mem),
                             (msg->raw_imu[0].utime - msg->raw_imu[1].utime) * 1E-6 };
      return processMessageAtlasPacket(&m, est);
    }
    if (msg->mem == PB_HOST_BROADCAST) {
      // one robot for every filter: de-duplicate and filter ONCE on the host (IIRNotch above), hand the newest filtered
      // packet over as a broadcast block.  (Do not mix with per-filter messages in one run: that state lives on the device.)
      if (host_notch_.empty())
        for (int ax = 0; ax < 3; ax++)
          for (int i = 0; i < 3; i++) host_notch_.emplace_back(notch_freq * (double) (1 << i), 1000.0);  // :33-40: f, 2f, 4f
      IMUBatch batch = imu_data_.convertFromLCMBatch(msg);
      if (batch.packets.empty()) return nullptr;
      double filt[3] = { 0, 0, 0 };
      for (const IMUPacket &pk : batch.packets)
        for (int ax = 0; ax < 3; ax++) {
          double v = pk.linear_acceleration[ax];
          for (int i = 0; i < 3; i++) v = host_notch_[(size_t) ax * 3 + i].processSample(v);
          filt[ax] = v;
        }
      const IMUPacket &p = batch.packets.back();
      msgs::kvh_raw_imu_t m{ msg->utime, BatchArray(p.delta_rotation, PB_HOST_BROADCAST), BatchArray(filt, PB_HOST_BROADCAST),
                             p.utime_delta * 1E-6 };
      return processMessageAtlasPacket(&m, est);
    }
    initNotch(est);
    IMUBatch batch = imu_data_.convertFromLCMBatch(msg);
    if (batch.packets.empty()) return nullptr;  // :181-187 "happens all the time at 1kHz"
    const size_t np = batch.packets.size();
    std::vector<double> acc((size_t) np * 3 * B), filt((size_t) 3 * B);
    for (size_t p = 0; p < np; p++) memcpy(&acc[p * 3 * B], batch.packets[p].linear_acceleration, sizeof(double) * 3 * B);
    if (pb_imu_notch(est->ctx, (int) np, acc.data(), filt.data(), PB_HOST) != PB_OK) return pb_report("InsHandler", est->ctx);
    const IMUPacket &p = batch.packets.back();  // the most recent filtered packet (:191-196)
    msgs::kvh_raw_imu_t m{ msg->utime, BatchArray(p.delta_rotation, PB_HOST), BatchArray(filt.data(), PB_HOST),
                           p.utime_delta * 1E-6 };
    return processMessageAtlasPacket(&m, est);
  }

  double notch_freq = 0.0;
  bool notch_initialised = false;
  // the device-side cascade (one state per filter), once
  void initNotch(MavStateEstimator *est)
  {
    if (notch_initialised) return;
    if (pb_imu_notch_init(est->ctx, notch_freq, 1000) != PB_OK) pb_report_exit("InsHandler", est->ctx);  // fs = 1000 (:32)
    notch_initialised = true;
  }
  IMUStream imu_data_;
  std::vector<IIRNotch> host_notch_;  // [axis][stage], broadcast messages only

  // Microstrain path (sensor_handlers.cpp:96-131): rotate accel and gyro into the body frame, dt = param
  RBISUpdateInterface *processMessage(const msgs::ins_t *msg, MavStateEstimator *est)
  {
    if (msg->gyro.mem == PB_DEVICE && msg->accel.mem == PB_DEVICE)   // per-filter samples already in HBM: the frame rotation runs there
      return buildOnDevice(est, msg->gyro.p, msg->accel.p, nullptr, nullptr, msg->utime, msg->valid, false, PB_DEVICE);
    return build(msg->gyro, msg->accel, 1.0, false, dt, msg->utime, est->B, msg->valid);
  }
  // Atlas KVH path for B DIFFERENT robots (independent log segments): the de-duplication ran per robot where the messages were
  // decoded (msgs::kvh_raw_imu_segments_t); here the notch cascade of every filter takes ITS new packets (pb_imu_notch_counts), and
  // the newest filtered packet becomes the process step with the filter's own raw_dt and its own message-time dt
  // (sensor_handlers.cpp:173-252).  A filter without a new packet -- the reference returns NULL for its message -- idles (dt = 0).
  // Returns NULL when the message carries nothing at all (max_new == 0).
  RBISUpdateInterface *processMessageAtlasSegments(const msgs::kvh_raw_imu_segments_t *msg, MavStateEstimator *est)
  {
    if ((msg->mem != PB_HOST && msg->mem != PB_DEVICE) || msg->max_new < 1 || !msg->new_accel || !msg->delta_rotation || !msg->raw_dt) return nullptr;
    const size_t B = (size_t) est->B;
    const double *accel = msg->new_accel;   // atlas_filter == false: row 0 is the newest packet, unfiltered (:199-204)
    if (atlas_filter) {
      initNotch(est);
      if (msg->n_new == nullptr) return nullptr;
      if (msg->mem == PB_DEVICE && notch_out_dev_ == nullptr) {
        void *d = nullptr;
        if (pb_malloc(est->ctx, sizeof(double) * 3 * B, &d) != PB_OK) pb_report_exit("InsHandler", est->ctx);
        notch_out_dev_ = std::make_shared<DeviceBlock>(std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(double) * 3 * B), d);
      }
      if (msg->mem == PB_HOST) notch_out_host_.resize(3 * B);
      double *filtered = msg->mem == PB_DEVICE ? (double *) notch_out_dev_->p : notch_out_host_.data();
      if (pb_imu_notch_counts(est->ctx, msg->max_new, msg->n_new, msg->new_accel, filtered, msg->mem) != PB_OK) return pb_report("InsHandler", est->ctx);
      accel = filtered;
    }
    return buildOnDevice(est, msg->delta_rotation, accel, msg->raw_dt, msg->utimes, msg->utime, msg->valid, true, msg->mem);
  }
  // Atlas KVH path without the notch (sensor_handlers.cpp:199-252): gyro = delta_rotation/raw_dt, accel through the
  // full ins_to_body transform (rotation + translation, :227), dt from message timestamps (:239-249)
  RBISUpdateInterface *processMessageAtlasPacket(const msgs::kvh_raw_imu_t *msg, MavStateEstimator *est)
  {
    double integration_dt = (prev_utime_atlas == 0) ? dt : (msg->utime - prev_utime_atlas) * 1E-6;
    if (integration_dt > 0.1) fprintf(stdout, "dt was : %f - there is an issue with timestamps\n", integration_dt);
    prev_utime_atlas = msg->utime;
    return build(msg->delta_rotation, msg->linear_acceleration, 1.0 / msg->raw_dt, true, integration_dt, msg->utime, est->B);
  }

  // ---- initialisation from gravity (processMessageInit / processMessageInitCommon, sensor_handlers.cpp:254-364) ----
  // Averages num_to_init body-frame IMU samples per filter: roll and pitch from the mean specific force
  // (init quat = init quat * setFromTwoVectors(mean(-accel), -z)), the gyro bias from the mean rate (0 if any axis exceeds
  // max_initial_gyro_bias), the matching covariance blocks from default_cov.  As in the reference the INS goes last
  // (allInitializedExcept "ins") and the bias that ends up in init_state is *_bias_initial -- the estimate only if
  // *_bias_recalc_at_start.  When the filter also initialises with "gps", the yaw comes from the mean magnetometer vector
  // (msgs::ins_t::mag, moved to the body frame with bot_trans_apply_vec like :148): its horizontal part is turned onto +y
  // (ENU, :338-351).  Keys are read (or_fail) on first use.
  int num_to_init = 0, init_counter = 0;
  double max_initial_gyro_bias = 0;
  bool accel_bias_recalc_at_start = false, gyro_bias_recalc_at_start = false;
  std::vector<double> g_vec_sum, gyro_bias_sum, mag_vec_sum;  // [3][B]
  std::vector<double> gyro_bias_initial, accel_bias_initial;  // [3] (same for every filter) or [3][B] after a recalc
  bool processMessageInit(const msgs::ins_t *msg, const std::map<std::string, bool> &sensors_initialized,
                          const RBIS & /*default_state*/, const RBIM &default_cov, RBIS &init_state, RBIM &init_cov)
  {
    const int B = init_state.B, n = init_state.n;
    if (!init_params_read_) {
      num_to_init = (int) bot_param_get_int_or_fail(param_, "state_estimator.ins.num_to_init");
      max_initial_gyro_bias = bot_param_get_double_or_fail(param_, "state_estimator.ins.max_initial_gyro_bias");
      gyro_bias_initial.resize(3);
      accel_bias_initial.resize(3);
      bot_param_get_double_array_or_fail(param_, "state_estimator.ins.accel_bias_initial", accel_bias_initial.data(), 3);
      bot_param_get_double_array_or_fail(param_, "state_estimator.ins.gyro_bias_initial", gyro_bias_initial.data(), 3);
      accel_bias_recalc_at_start = bot_param_get_boolean_or_fail(param_, "state_estimator.ins.accel_bias_recalc_at_start");
      gyro_bias_recalc_at_start = bot_param_get_boolean_or_fail(param_, "state_estimator.ins.gyro_bias_recalc_at_start");
      g_vec_sum.assign((size_t) 3 * B, 0.0);
      gyro_bias_sum.assign((size_t) 3 * B, 0.0);
      mag_vec_sum.assign((size_t) 3 * B, 0.0);
      init_params_read_ = true;
    }
    init_state.utime = msg->utime;
    auto *update = static_cast<RBISIMUProcessStep *>(build(msg->gyro, msg->accel, 1.0, false, dt, msg->utime, B));
    if (update == nullptr) return false;
    if (!RBISInitializer::allInitializedExcept(sensors_initialized, "ins")) {  // force the INS to go last (:266-267)
      delete update;
      return false;
    }
    init_counter++;
    const size_t per = batch_per(update->imu_block.mem, B);
    for (int b = 0; b < B; b++) {
      const size_t sb = (per == 1) ? 0 : (size_t) b;
      for (int i = 0; i < 3; i++) {
        gyro_bias_sum[(size_t) i * B + b] += update->owned[(size_t) i * per + sb];            // :291
        g_vec_sum[(size_t) i * B + b] += -update->owned[(size_t) (3 + i) * per + sb];         // :289
      }
    }
    delete update;
    if (msg->mag.p != nullptr && msg->mag.mem != PB_DEVICE) {  // :147-149, :290
      const size_t mper = batch_per(msg->mag.mem, B);
      for (int b = 0; b < B; b++) {
        const size_t sb = (mper == 1) ? 0 : (size_t) b;
        const double ms[3] = { msg->mag.p[sb], msg->mag.p[mper + sb], msg->mag.p[2 * mper + sb] };
        double mb[3];
        bot_trans_apply_vec(&ins_to_body, ms, mb);
        for (int i = 0; i < 3; i++) mag_vec_sum[(size_t) i * B + b] += mb[i];
      }
    }
    if (init_counter < num_to_init) return false;
    bool warned = false;
    std::vector<double> gb_est((size_t) 3 * B);
    for (int b = 0; b < B; b++) {
      if (!warned && (init_cov(RBIS::chi_ind, RBIS::chi_ind, b) > 0 || init_cov(RBIS::chi_ind + 1, RBIS::chi_ind + 1, b) > 0)) {
        fprintf(stderr, "Warning: overriding initial roll, pitch with IMU values\n");
        warned = true;
      }
      double g_est[3], gb[3];
      bool too_big = false;
      for (int i = 0; i < 3; i++) {
        g_est[i] = g_vec_sum[(size_t) i * B + b] / (double) init_counter;
        gb[i] = gyro_bias_sum[(size_t) i * B + b] / (double) init_counter;
        too_big = too_big || fabs(gb[i]) > max_initial_gyro_bias;
      }
      if (too_big) gb[0] = gb[1] = gb[2] = 0.0;                                                 // :303-311
      const double minus_z[3] = { 0.0, 0.0, -1.0 };
      double qg[4];
      quat_from_two_vectors(g_est, minus_z, qg);                                               // :314-315
      const double q0[4] = { init_state.q(0, b), init_state.q(1, b), init_state.q(2, b), init_state.q(3, b) };
      double qn[4];
      quat_mult(q0, qg, qn);
      for (int i = 0; i < 4; i++) init_state.q(i, b) = qn[i];                                   // :320
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 2; c++)
          init_cov(RBIS::chi_ind + r, RBIS::chi_ind + c, b) = default_cov(RBIS::chi_ind + r, RBIS::chi_ind + c, b);  // :321-322
      if (n == RBIS::rbis_num_states)
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++)
            init_cov(RBIS::gyro_bias_ind + r, RBIS::gyro_bias_ind + c, b) = default_cov(RBIS::gyro_bias_ind + r, RBIS::gyro_bias_ind + c, b);
      for (int i = 0; i < 3; i++) gb_est[(size_t) i * B + b] = gb[i];
      if (RBISInitializer::initializingWith(sensors_initialized, "gps")) {                      // :338-351
        double m_est[3] = { mag_vec_sum[b] / (double) init_counter, mag_vec_sum[(size_t) B + b] / (double) init_counter, 0.0 };
        const double unit_y[3] = { 0.0, 1.0, 0.0 };  // "in ENU, the magnetic vector should be aligned with Y axis"
        double qm[4];
        quat_from_two_vectors(m_est, unit_y, qm);
        const double q1[4] = { init_state.q(0, b), init_state.q(1, b), init_state.q(2, b), init_state.q(3, b) };
        double qy[4];
        quat_mult(qm, q1, qy);
        for (int i = 0; i < 4; i++) init_state.q(i, b) = qy[i];                                 // quat_mag * orientation
        init_cov(RBIS::chi_ind + 2, RBIS::chi_ind + 2, b) = default_cov(RBIS::chi_ind + 2, RBIS::chi_ind + 2, b);
      }
    }
    if (accel_bias_recalc_at_start && n == RBIS::rbis_num_states) {  // :353-356: whatever init_state holds now
      accel_bias_initial.resize((size_t) 3 * B);
      for (int b = 0; b < B; b++)
        for (int i = 0; i < 3; i++) accel_bias_initial[(size_t) i * B + b] = init_state(RBIS::accel_bias_ind + i, b);
    }
    if (gyro_bias_recalc_at_start) gyro_bias_initial = gb_est;     // :358-361
    if (n == RBIS::rbis_num_states) {
      for (int b = 0; b < B; b++)
        for (int i = 0; i < 3; i++) {                               // :363-364
          init_state(RBIS::gyro_bias_ind + i, b) = gyro_bias_initial[gyro_bias_initial.size() == 3 ? (size_t) i : (size_t) i * B + b];
          init_state(RBIS::accel_bias_ind + i, b) = accel_bias_initial[accel_bias_initial.size() == 3 ? (size_t) i : (size_t) i * B + b];
        }
    }
    return true;
  }

private:
  BotParam *param_ = nullptr;
  bool init_params_read_ = false;
  std::shared_ptr<DevicePool> ins_pool_;         // [7][B] process-step blocks made on the device
  std::shared_ptr<DeviceBlock> notch_out_dev_;   // [3][B] newest filtered packet (stream order: read by the step made from it)
  std::vector<double> notch_out_host_;
  // The per-sample arithmetic of processMessage / processMessageAtlas for B robots on the device (pb_ins_body_block): the update
  // owns the [7][B] block it is given.  atlas: gyro holds delta_rotation (divided by raw_dt), the acceleration is translated too,
  // dt comes from every filter's own message times.
  RBISUpdateInterface *buildOnDevice(MavStateEstimator *est, const double *gyro, const double *accel, const double *raw_dt, const int64_t *utimes,
                                     int64_t utime, const uint8_t *valid, bool atlas, int mem)
  {
    if (!ins_pool_) ins_pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(double) * 7 * (size_t) est->B + (size_t) est->B);
    const std::shared_ptr<DeviceBlock> block = take_block(ins_pool_);   // (unused, it goes back to the pool when this call fails)
    void *blk = block ? block->p : nullptr;
    // (the block is [7][B] doubles + a [B] mask behind it: the update OWNS its copy of the mask -- a host mask is gone when the handler
    // returns, and a device mask inside a replayer's chunk buffer may be overwritten before a held-back step has run)
    uint8_t *mask_out = (blk != nullptr && valid != nullptr) ? (uint8_t *) ((double *) blk + (size_t) 7 * est->B) : nullptr;
    if (blk == nullptr ||
        pb_ins_body_block(est->ctx, gyro, accel, raw_dt, utimes, utime, valid, ins_to_body.rot_quat, atlas ? ins_to_body.trans_vec : nullptr, dt,
                          atlas ? 1 : 0, mem, (double *) blk, mask_out) != PB_OK)
      return pb_report("InsHandler", est->ctx);
    auto *u = new RBISIMUProcessStep(BatchArray((const double *) blk, PB_DEVICE), cov_gyro, cov_accel, cov_gyro_bias, cov_accel_bias, utime);
    u->owned_dev = block;
    u->valid_dev = mask_out;
    u->may_idle = mask_out != nullptr && (mem != PB_HOST || std::find(valid, valid + est->B, (uint8_t) 0) != valid + est->B);
    return u;
  }
  // valid [B] (per-filter host messages only): a filter without a message takes its step with dt = 0 -- with the sample it was
  // handed (its own last one) that leaves its state and covariance where they are
  RBISUpdateInterface *build(BatchArray gyro, BatchArray accel, double gyro_scale, bool accel_translate, double dt_,
                             int64_t utime, int B, const uint8_t *valid = nullptr)
  {
    if (gyro.mem == PB_DEVICE || accel.mem == PB_DEVICE || gyro.mem != accel.mem) {
      fprintf(stderr, "InsHandler: sensor-frame inputs must be host arrays (frame rotation is a host pass)\n");
      return nullptr;
    }
    // PB_HOST_BROADCAST: one IMU for every filter -> rotate once, hand a [7] block over (expanded on the device)
    const int mem = gyro.mem;
    if (mem == PB_HOST_BROADCAST) B = 1;
    std::vector<double> blk((size_t) 7 * B);
    const bool ident = ins_to_body.isIdentityRotation();
    PB_SHIM_PARALLEL_FOR
    for (int b = 0; b < B; b++) {
      double g[3] = { gyro.p[b] * gyro_scale, gyro.p[(size_t) B + b] * gyro_scale, gyro.p[(size_t) 2 * B + b] * gyro_scale };
      double a[3] = { accel.p[b], accel.p[(size_t) B + b], accel.p[(size_t) 2 * B + b] };
      double gb[3], ab[3];
      if (ident) {
        memcpy(gb, g, sizeof g);
        memcpy(ab, a, sizeof a);
      } else {
        bot_quat_rotate_to(ins_to_body.rot_quat, g, gb);
        bot_quat_rotate_to(ins_to_body.rot_quat, a, ab);
      }
      if (accel_translate)
        for (int i = 0; i < 3; i++) ab[i] += ins_to_body.trans_vec[i];
      for (int i = 0; i < 3; i++) {
        blk[(size_t) i * B + b] = gb[i];
        blk[(size_t) (3 + i) * B + b] = ab[i];
      }
      blk[(size_t) 6 * B + b] = (valid != nullptr && mem == PB_HOST && !valid[b]) ? 0.0 : dt_;
    }
    auto *u = new RBISIMUProcessStep(std::move(blk), cov_gyro, cov_accel, cov_gyro_bias, cov_accel_bias, utime, mem);
    if (valid != nullptr && mem == PB_HOST) {
      u->valid_host.assign(valid, valid + B);
      u->may_idle = std::find(valid, valid + B, (uint8_t) 0) != valid + B;
    }
    return u;
  }
};

// pronto_math.cpp:25-61 and pronto_conversions_lcm.hpp:38-87
inline void quat_to_euler(const double q[4], double &roll, double &pitch, double &yaw)
{
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  roll = atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2));
  pitch = asin(2 * (q0 * q2 - q3 * q1));
  yaw = atan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3));
}

class LegOdoCommon {
public:
  typedef enum { MODE_LIN_RATE, MODE_ROT_RATE, MODE_LIN_AND_ROT_RATE, MODE_POSITION_AND_LIN_RATE } LegOdoCommonMode;
  LegOdoCommonMode mode_;
  double R_legodo_xyz_, R_legodo_vxyz_, R_legodo_vang_, R_legodo_vxyz_uncertain_, R_legodo_vang_uncertain_;

  explicit LegOdoCommon(BotParam *param)
  {
    std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.legodo.mode");
    if (mode_str == "lin_rot_rate") mode_ = MODE_LIN_AND_ROT_RATE;
    else if (mode_str == "lin_rate") mode_ = MODE_LIN_RATE;
    else if (mode_str == "pos_and_lin_rate") mode_ = MODE_POSITION_AND_LIN_RATE;
    else {
      fprintf(stdout, "Legodo not understood! [LegOdoCommon].\n");  // rbis_legodo_common.cpp:19-21 (mode_ left unset there)
      mode_ = MODE_LIN_RATE;
    }
    R_legodo_xyz_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.r_xyz");
    R_legodo_vxyz_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.r_vxyz");
    R_legodo_vang_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.r_vang");
    R_legodo_vxyz_uncertain_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.r_vxyz_uncertain");
    R_legodo_vang_uncertain_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.r_vang_uncertain");
  }

  // getCovariance (rbis_legodo_common.cpp:34-88) for one filter: fills Rdiag[m], z_indices; returns m
  // getCovariance (rbis_legodo_common.cpp:34-91): diagonal of R and, if asked for, the index list
  int getCovariance(LegOdoCommonMode mode_current, bool delta_certain, double *Rdiag, std::vector<int> *z_indices) const
  {
    const double rv = delta_certain ? R_legodo_vxyz_ : R_legodo_vxyz_uncertain_;
    const double ra = delta_certain ? R_legodo_vang_ : R_legodo_vang_uncertain_;
    if (mode_current == MODE_LIN_AND_ROT_RATE) {
      for (int i = 0; i < 3; i++) { Rdiag[i] = bot_sq(rv); Rdiag[3 + i] = bot_sq(ra); }
      if (z_indices) *z_indices = { 3, 4, 5, 0, 1, 2 };
      return 6;
    } else if (mode_current == MODE_POSITION_AND_LIN_RATE) {
      for (int i = 0; i < 3; i++) { Rdiag[i] = bot_sq(R_legodo_xyz_); Rdiag[3 + i] = bot_sq(rv); }
      if (z_indices) *z_indices = { 9, 10, 11, 3, 4, 5 };
      return 6;
    }
    for (int i = 0; i < 3; i++) Rdiag[i] = bot_sq(rv);
    if (z_indices) *z_indices = { 3, 4, 5 };
    return 3;
  }

  // createMeasurement (rbis_legodo_common.cpp:110-169) for B filters.  Filters whose delta status is < 0 (the
  // handler's "return NULL", rbis_legodo_update.cpp:242-255) get mask 0.  In mode pos_and_lin_rate the reference
  // falls back to lin_rate per message when the position is invalid (:118-122): those filters take an m = 3 velocity
  // update, the others the m = 6 one (RBISEitherUpdate), so every filter gets exactly the reference's update and
  // log-likelihood increment.
  RBISUpdateInterface *createMeasurement(const msgs::legodo_delta_t *msg, int B) const
  {
    if (mode_ == MODE_POSITION_AND_LIN_RATE && msg->position_status != nullptr) {
      bool any_bad = false, any_good = false;
      for (int b = 0; b < B; b++) (msg->position_status[b] ? any_good : any_bad) = true;
      if (any_bad) {
        LegOdoCommon lin(*this);
        lin.mode_ = MODE_LIN_RATE;
        msgs::legodo_delta_t m3 = *msg;
        m3.position_status = nullptr;
        auto *fallback = static_cast<RBISIndexedMeasurement *>(lin.createMeasurement(&m3, B));
        for (int b = 0; b < B; b++) fallback->owned_mask[(size_t) b] &= (uint8_t) !msg->position_status[b];
        if (!any_good) return fallback;
        msgs::legodo_delta_t m6 = *msg;
        m6.position_status = nullptr;
        auto *full = static_cast<RBISIndexedMeasurement *>(createMeasurement(&m6, B));
        for (int b = 0; b < B; b++) full->owned_mask[(size_t) b] &= (uint8_t) (msg->position_status[b] != 0);
        return new RBISEitherUpdate(full, fallback);
      }
    }
    const double elapsed = (double) (msg->utime - msg->prev_utime) * 1E-6;  // pronto_conversions_lcm.hpp:45
    const int m = (mode_ == MODE_LIN_RATE) ? 3 : 6;
    std::vector<double> z((size_t) m * B), R((size_t) m * B);
    std::vector<uint8_t> mask(B);
    std::vector<int> idx;
    {
      double unused[6];
      getCovariance(mode_, true, unused, &idx);
    }
    PB_SHIM_PARALLEL_FOR
    for (int b = 0; b < B; b++) {
      const float st = msg->delta_status ? msg->delta_status[b] : 0.f;
      mask[b] = st >= 0;
      const bool certain = st < 0.5;                                        // :124-129
      double Rd[6];
      getCovariance(mode_, certain, Rd, nullptr);
      double vel[3];
      for (int i = 0; i < 3; i++) vel[i] = msg->delta_trans[(size_t) i * B + b] / elapsed;   // getDeltaAsVelocity :73
      if (mode_ == MODE_LIN_RATE) {
        for (int i = 0; i < 3; i++) { z[(size_t) i * B + b] = vel[i]; R[(size_t) i * B + b] = Rd[i]; }
      } else if (mode_ == MODE_LIN_AND_ROT_RATE) {
        double q[4] = { 1, 0, 0, 0 }, rpy[3];
        if (msg->delta_quat) for (int i = 0; i < 4; i++) q[i] = msg->delta_quat[(size_t) i * B + b];
        quat_to_euler(q, rpy[0], rpy[1], rpy[2]);                           // :141-147
        for (int i = 0; i < 3; i++) {
          z[(size_t) i * B + b] = vel[i];
          z[(size_t) (3 + i) * B + b] = rpy[i] / (((double) msg->utime - msg->prev_utime) / 1000000);
          R[(size_t) i * B + b] = Rd[i];
          R[(size_t) (3 + i) * B + b] = Rd[3 + i];
        }
      } else {
        for (int i = 0; i < 3; i++) {
          z[(size_t) i * B + b] = msg->position ? msg->position[(size_t) i * B + b] : 0.0;
          z[(size_t) (3 + i) * B + b] = vel[i];
          R[(size_t) i * B + b] = Rd[i];
          R[(size_t) (3 + i) * B + b] = Rd[3 + i];
        }
      }
    }
    return new RBISIndexedMeasurement(idx, std::move(z), std::move(R), PB_R_DIAG, std::move(mask),
                                      RBISUpdateInterface::legodo, msg->utime);
  }
};

// ModelClient (the reference hands its URDF string to kdl_parser, leg_estimate.cpp:68-73): here it carries what the
// forward kinematics of the two standing links needs of the robot model -- per leg the joints from the root link down to
// the standing link with their <origin>, <axis> and type -- filled in by hand or by fromURDFString(), a reader for exactly
// those URDF elements (<joint name type> with <parent link>, <child link>, <origin xyz rpy>, <axis xyz>).
class ModelClient {
public:
  struct Joint {
    std::string name;
    int type = 1;  // 0 fixed, 1 revolute / continuous, 2 prismatic (pb_legodo_set_chain)
    double xyz[3] = { 0, 0, 0 }, rpy[3] = { 0, 0, 0 }, axis[3] = { 1, 0, 0 };  // (URDF defaults)
  };
  std::vector<Joint> left_chain, right_chain;
  std::string urdf;
  std::string getURDFString() const { return urdf; }

  // the chain of joints from the root link to `link`; false if the link is not the child of any joint, a joint type is
  // not one the chain table knows (floating, planar), or an <origin> / <axis> attribute does not parse
  static bool chainTo(const std::string &urdf_with_comments, const std::string &link, std::vector<Joint> &chain)
  {
    struct J { Joint j; std::string parent, child; };
    std::vector<J> all;
    std::string urdf_xml;  // without <!-- comments -->: a commented-out joint must not be read
    for (size_t p = 0; p < urdf_with_comments.size();) {
      const size_t c0 = urdf_with_comments.find("<!--", p);
      urdf_xml.append(urdf_with_comments, p, (c0 == std::string::npos ? urdf_with_comments.size() : c0) - p);
      if (c0 == std::string::npos) break;
      const size_t c1 = urdf_with_comments.find("-->", c0 + 4);
      if (c1 == std::string::npos) break;
      p = c1 + 3;
    }
    // name = "value" (XML allows white space around '='; either quote)
    auto attr = [](const std::string &tag, const char *name, std::string &out) {
      const std::string key(name);
      auto space = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r'; };
      size_t p = 0;
      while ((p = tag.find(key, p)) != std::string::npos) {
        const bool starts_word = p == 0 || !(isalnum((unsigned char) tag[p - 1]) || tag[p - 1] == '_' || tag[p - 1] == ':');
        p += key.size();
        if (!starts_word) continue;
        size_t v = p;
        while (v < tag.size() && space(tag[v])) v++;
        if (v >= tag.size() || tag[v] != '=') continue;
        v++;
        while (v < tag.size() && space(tag[v])) v++;
        if (v >= tag.size() || (tag[v] != '"' && tag[v] != '\'')) continue;
        const char qc = tag[v];
        const size_t e = tag.find(qc, v + 1);
        if (e == std::string::npos) return false;
        out = tag.substr(v + 1, e - v - 1);
        return true;
      }
      return false;
    };
    // exactly three numbers (urdfdom's Vector3::init throws on anything else; the reference exits when kdl_parser fails)
    auto three = [](const std::string &v, double *o) {
      char extra;
      return sscanf(v.c_str(), " %lf %lf %lf %c", o, o + 1, o + 2, &extra) == 3;
    };
    size_t pos = 0;
    while ((pos = urdf_xml.find("<joint", pos)) != std::string::npos) {
      const size_t head_end = urdf_xml.find('>', pos);
      if (head_end == std::string::npos) break;
      const std::string head = urdf_xml.substr(pos, head_end - pos + 1);
      const char nx = urdf_xml[pos + 6];
      if (!(nx == ' ' || nx == '\t' || nx == '\n' || nx == '\r')) { pos = head_end; continue; }  // e.g. <joint_properties>
      std::string type;
      J j;
      if (!attr(head, "name", j.j.name) || !attr(head, "type", type) || head[head.size() - 2] == '/') { pos = head_end; continue; }  // (a <transmission>'s <joint name=.../>)
      const size_t end = urdf_xml.find("</joint>", head_end);
      if (end == std::string::npos) break;
      const std::string body = urdf_xml.substr(head_end + 1, end - head_end - 1);
      pos = end;
      j.j.type = (type == "fixed") ? 0 : (type == "revolute" || type == "continuous") ? 1 : (type == "prismatic") ? 2 : -1;
      auto child_tag = [&](const char *name, std::string &tag) {
        const size_t p = body.find(std::string("<") + name);
        if (p == std::string::npos) return false;
        const size_t e = body.find('>', p);
        if (e == std::string::npos) return false;
        tag = body.substr(p, e - p + 1);
        return true;
      };
      std::string tag, v;
      if (!child_tag("parent", tag) || !attr(tag, "link", j.parent)) continue;
      if (!child_tag("child", tag) || !attr(tag, "link", j.child)) continue;
      // an <origin> / <axis> attribute that is present but does not hold three numbers is an error, not a default
      if (child_tag("origin", tag)) {
        if (attr(tag, "xyz", v) && !three(v, j.j.xyz)) return false;
        if (attr(tag, "rpy", v) && !three(v, j.j.rpy)) return false;
      }
      if (child_tag("axis", tag) && attr(tag, "xyz", v) && !three(v, j.j.axis)) return false;
      all.push_back(j);
    }
    chain.clear();
    std::string cur = link;
    for (size_t guard = 0; guard <= all.size(); guard++) {
      const J *up = nullptr;
      for (const J &j : all)
        if (j.child == cur) up = &j;
      if (up == nullptr) break;  // cur is the root link
      if (up->j.type < 0) return false;
      chain.insert(chain.begin(), up->j);
      cur = up->parent;
    }
    return !chain.empty();
  }
  bool fromURDFString(const std::string &urdf_xml, const std::string &left_standing_link, const std::string &right_standing_link)
  {
    urdf = urdf_xml;
    return chainTo(urdf_xml, left_standing_link, left_chain) && chainTo(urdf_xml, right_standing_link, right_chain);
  }
};

// LegOdoHandler (rbis_legodo_update.cpp:10-280).  processMessage(joint_state_t) is the reference's handler: torque
// adjustment, forward kinematics, leg_estimate::updateOdometry and LegOdoCommon::createMeasurement -- all of it per filter
// on the device, because its world_to_body_ is the filter's own head pose (:214-229).  processMessageFeet takes the two
// body-to-foot transforms instead of the joint angles (a caller with its own kinematics), processMessageDelta the finished
// increment.
class LegOdoHandler {
public:
  LegOdoCommon *leg_odo_common_;
  int zero_initial_velocity;      // rbis_legodo_update.cpp:58,265-269
  bool force_torque_init_ = true; // rbis_legodo_update.cpp:98,197,208-211: nothing is integrated before the first
                                  // force/torque message; the joint-state path starts with false like the reference (its foot
                                  // forces come from forceTorqueHandler); the increment / foot-state paths, whose callers
                                  // already hold the foot sensing, start with true
  explicit LegOdoHandler(BotParam *param) : leg_odo_common_(new LegOdoCommon(param)), zero_initial_velocity(0), param_(param)
  {
    zero_initial_velocity = bot_param_get_int_or(param, "state_estimator.legodo.zero_initial_velocity", zero_initial_velocity);
  }
  // the reference's constructor (lcm_recv, lcm_pub, param, model, frames) without the LCM objects and BotFrames
  LegOdoHandler(BotParam *param, const ModelClient *model) : LegOdoHandler(param)
  {
    model_ = model;
    force_torque_init_ = false;
    // leg_estimate's constructor (leg_estimate.cpp:29-142)
    const std::string init_mode = bot_param_get_str_or_fail(param, "state_estimator.legodo.initialization_mode");
    if (init_mode != "zero") fprintf(stdout, "Leg Odometry Initialize Mode: %s (only \"zero\" moves the pose, leg_estimate.cpp:172-190)\n", init_mode.c_str());
    // leg_estimate.cpp:43-61: "lowpass" | "kalman" | anything else = no filtering
    const std::string filt = bot_param_get_str_or_fail(param, "state_estimator.legodo.filter_joint_positions");
    if (filt == "lowpass") {
      filter_joint_positions_ = 1;
    } else if (filt == "kalman") {
      filter_joint_positions_ = 2;
      joint_process_noise_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.joint_process_noise");
      joint_observation_noise_ = bot_param_get_double_or_fail(param, "state_estimator.legodo.joint_observation_noise");
    }
    use_torque_adjustment_ = bot_param_get_boolean_or_fail(param, "state_estimator.legodo.torque_adjustment");
    if (use_torque_adjustment_) {  // rbis_legodo_update.cpp:29-53
      const std::string &names = bot_param_get_raw_or_fail(param, "state_estimator.legodo.adjustment_joints");
      size_t p = 0;
      while (p < names.size()) {
        while (p < names.size() && (names[p] == ' ' || names[p] == ',' || names[p] == '[' || names[p] == ']' || names[p] == '"')) p++;
        size_t e = p;
        while (e < names.size() && names[e] != ' ' && names[e] != ',' && names[e] != ']' && names[e] != '"') e++;
        if (e > p) adjustment_joints_.push_back(names.substr(p, e - p));
        p = e;
      }
      std::vector<double> g(adjustment_joints_.size());
      bot_param_get_double_array_or_fail(param, "state_estimator.legodo.adjustment_gain", g.data(), (int) g.size());
      for (double v : g) adjustment_gain_.push_back((float) v);
    }
  }
  ~LegOdoHandler() { delete leg_odo_common_; }
  void forceTorqueHandler() { force_torque_init_ = true; }
  // rbis_legodo_update.cpp:208-211: the gate in front of every entry point
  bool forceTorqueSeen() const
  {
    if (!force_torque_init_) fprintf(stdout, "Force/Torque message not received yet, not integrating leg odometry =========================\n");
    return force_torque_init_;
  }
  // rbis_legodo_update.cpp:195-204: keep the last force/torque message; processMessage reads |force z| of the two feet
  void forceTorqueHandler(const msgs::six_axis_force_torque_array_t *msg, int B)
  {
    const size_t n = (msg->force_z.mem == PB_HOST_BROADCAST) ? 2 : (size_t) 2 * B;
    foot_force_.resize(n);
    for (size_t i = 0; i < n; i++) foot_force_[i] = (float) fabs(msg->force_z.p[i]);  // FootSensing(fabs(...)) (:234-235), float members
    foot_force_mem_ = (msg->force_z.mem == PB_HOST_BROADCAST) ? PB_HOST_BROADCAST : PB_HOST;
    foot_force_dev_ = nullptr;
    force_torque_init_ = true;
  }
  // device-resident replays: |force z| [2][B] floats in HBM.  Like the device arrays of a PB_DEVICE joint_state_t it must stay
  // valid until the update made from it has been APPLIED: with fuse_ins_legodo the odometry of a message runs inside the pair
  // kernel of the addUpdate call that follows processMessage (same dispatch, FrontEnd::addSensor), so "until the next message"
  // is enough -- the estimator makes a deferred measurement at once whenever it holds the pair back or does not roll forward
  void forceTorqueDevice(const float *abs_force_z)
  {
    foot_force_dev_ = abs_force_z;
    force_torque_init_ = true;
  }
  // rbis_legodo_update.cpp:190-193
  void controllerInputHandler(const msgs::controller_foot_contact_t *msg)
  {
    n_control_contacts_[0] = msg->num_left_foot_contacts;
    n_control_contacts_[1] = msg->num_right_foot_contacts;
    control_contacts_dirty_ = true;
  }

  BotParam *param_ = nullptr;
  const ModelClient *model_ = nullptr;
  int filter_joint_positions_ = 0;   // 0 none, 1 lowpass, 2 kalman (leg_estimate.cpp:43-61)
  double joint_process_noise_ = 0, joint_observation_noise_ = 0;
  std::shared_ptr<DevicePool> jf_pool_;   // filtered joint blocks [rows][B] floats (per-filter joint states)
  std::shared_ptr<DevicePool> ff_pool_;   // foot forces [2][B] floats uploaded for device-resident joint blocks
  bool use_torque_adjustment_ = false;
  std::vector<std::string> adjustment_joints_;
  std::vector<float> adjustment_gain_;
  std::vector<float> foot_force_;
  int foot_force_mem_ = PB_HOST;
  const float *foot_force_dev_ = nullptr;
  int32_t n_control_contacts_[2] = { -1, -1 };
  bool control_contacts_dirty_ = false;
  std::shared_ptr<DevicePool> pool_;
  bool legodo_ready_ = false, chain_ready_ = false;
  std::vector<std::string> chain_names_;  // the joint_name list the chain rows were resolved against

  // leg_estimate's constructor parameters (leg_estimate.cpp:63,93-121) -> the device side, once
  void initLegEstimate(MavStateEstimator *est)
  {
    const int B = est->B;
    const double lt = bot_param_get_double_or_fail(param_, "state_estimator.legodo.schmitt_low_threshold");
    const double ht = bot_param_get_double_or_fail(param_, "state_estimator.legodo.schmitt_high_threshold");
    const int64_t ld = (int64_t) bot_param_get_double_or_fail(param_, "state_estimator.legodo.schmitt_low_delay");
    const int64_t hd = (int64_t) bot_param_get_double_or_fail(param_, "state_estimator.legodo.schmitt_high_delay");
    const bool fce = bot_param_get_boolean_or_fail(param_, "state_estimator.legodo.filter_contact_events");
    bool bad = pb_legodo_init(est->ctx, lt, ht, ld, hd, fce) != PB_OK;
    // the contact mode keys are read by leg_estimate's constructor, i.e. only when the handler was given a robot model
    if (!bad && model_ != nullptr) {
      const bool standing = bot_param_get_str_or_fail(param_, "state_estimator.legodo.init_contact_mode") == "standing";
      const double total_force = bot_param_get_double_or_fail(param_, "state_estimator.legodo.total_force");
      const double level = bot_param_get_double_or_fail(param_, "state_estimator.legodo.standing_schmitt_level");
      const bool ctrl = bot_param_get_boolean_or_fail(param_, "state_estimator.legodo.use_controller_input");
      bad = pb_legodo_set_contact_mode(est->ctx, standing, total_force, level, ctrl) != PB_OK;
    }
    // "ignore the calculated velocity at launch" is counted per filter on the device (valid ticks only, like :243-268)
    if (!bad) bad = pb_legodo_set_zero_initial_velocity(est->ctx, zero_initial_velocity) != PB_OK;
    if (bad) pb_report_exit("LegOdoHandler", est->ctx);
    // per update: the measurement block -- z and the diagonal of R, [6][B] (lin_rate) or [12][B] doubles -- and its mask(s) [2][B]
    pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(double) * 12 * (size_t) B + 2 * (size_t) B);
    legodo_ready_ = true;
    sweep_dirty_ = sweep_B_ != 0;   // (pb_legodo_init dropped the block)
  }
  // ---- parameter sweeps: the batch's form of the reference's `-O key=value` (state-estimator/python/param_sweep.py:39-52) ----
  // key: one of the eleven state_estimator.legodo.* names below (with or without that prefix); per_filter: its value for every filter
  // of the batch, in the .cfg's units.  The rows nobody swept hold the .cfg's value.  The first sweep fixes the batch size the
  // following ones must have; a wrong key or a wrong length returns false and changes nothing.  Takes effect with the next message
  // (pb_legodo_set_param_block); a length that is not the estimator's batch size ends the program there like every bad configuration.
  static const char *sweepKey(int row)
  {
    static const char *const keys[PB_LEGPAR_ROWS] = { "r_vxyz", "r_vxyz_uncertain", "r_vang", "r_vang_uncertain", "r_xyz", "schmitt_low_threshold",
                                                      "schmitt_high_threshold", "schmitt_low_delay", "schmitt_high_delay", "total_force",
                                                      "standing_schmitt_level" };
    return keys[row];
  }
  bool setSweep(const std::string &key, const std::vector<double> &per_filter)
  {
    const std::string prefix = "state_estimator.legodo.";
    const std::string k = key.compare(0, prefix.size(), prefix) == 0 ? key.substr(prefix.size()) : key;
    int row = -1;
    for (int r = 0; r < PB_LEGPAR_ROWS; r++)
      if (k == sweepKey(r)) row = r;
    if (row < 0 || per_filter.empty() || (sweep_B_ != 0 && per_filter.size() != sweep_B_)) return false;
    sweep_B_ = per_filter.size();
    sweep_rows_[row] = per_filter;
    sweep_dirty_ = true;
    return true;
  }
  size_t sweep_B_ = 0;
  std::vector<double> sweep_rows_[PB_LEGPAR_ROWS];
  bool sweep_dirty_ = false;
  void applySweep(MavStateEstimator *est)
  {
    const size_t B = (size_t) est->B;
    if (sweep_B_ != B) {
      fprintf(stderr, "LegOdoHandler: setSweep was given %zu values per key, the batch has %zu filters\n", sweep_B_, B);
      exit(1);
    }
    const LegOdoCommon *lc = leg_odo_common_;
    auto cfg = [&](int row) -> double {
      switch (row) {
      case PB_LEGPAR_R_VXYZ: return lc->R_legodo_vxyz_;
      case PB_LEGPAR_R_VXYZ_UNCERTAIN: return lc->R_legodo_vxyz_uncertain_;
      case PB_LEGPAR_R_VANG: return lc->R_legodo_vang_;
      case PB_LEGPAR_R_VANG_UNCERTAIN: return lc->R_legodo_vang_uncertain_;
      case PB_LEGPAR_R_XYZ: return lc->R_legodo_xyz_;
      default: break;
      }
      const std::string key = std::string("state_estimator.legodo.") + sweepKey(row);
      if (row == PB_LEGPAR_TOTAL_FORCE || row == PB_LEGPAR_STANDING_SCHMITT_LEVEL) {  // read only with a robot model (initLegEstimate)
        return model_ != nullptr ? bot_param_get_double_or(param_, key.c_str(), 0.0) : 0.0;
      }
      const double v = bot_param_get_double_or_fail(param_, key.c_str());
      return (row == PB_LEGPAR_SCHMITT_LOW_DELAY || row == PB_LEGPAR_SCHMITT_HIGH_DELAY) ? (double) (int64_t) v : v;
    };
    std::vector<double> block((size_t) PB_LEGPAR_ROWS * B);
    for (int row = 0; row < PB_LEGPAR_ROWS; row++) {
      if (sweep_rows_[row].empty()) std::fill(block.begin() + (size_t) row * B, block.begin() + (size_t) (row + 1) * B, cfg(row));
      else std::copy(sweep_rows_[row].begin(), sweep_rows_[row].end(), block.begin() + (size_t) row * B);
    }
    if (pb_legodo_set_param_block(est->ctx, block.data(), PB_HOST) != PB_OK) pb_report_exit("LegOdoHandler", est->ctx);
    sweep_dirty_ = false;
  }
  // fksolver_->JntToCart looks joints up by name (leg_estimate.cpp:432-436): resolve the chain's names against the message's
  void initChain(const msgs::joint_state_t *msg, MavStateEstimator *est)
  {
    std::vector<int> type, row;
    std::vector<double> org, axis;
    std::vector<float> gain;
    for (const std::vector<ModelClient::Joint> *chain : { &model_->left_chain, &model_->right_chain })
      for (const ModelClient::Joint &j : *chain) {
        int r = 0;
        if (j.type != 0) {
          const auto it = std::find(msg->joint_name.begin(), msg->joint_name.end(), j.name);
          if (it == msg->joint_name.end()) {  // KDL treats a missing joint as an error; the reference then exit(-1)s (:438-441)
            fprintf(stderr, "Error: could not calculate forward kinematics! (joint %s is not in the joint state)\n", j.name.c_str());
            exit(-1);
          }
          r = (int) (it - msg->joint_name.begin());
        }
        type.push_back(j.type);
        row.push_back(r);
        for (int i = 0; i < 3; i++) org.push_back(j.xyz[i]);
        for (int i = 0; i < 3; i++) org.push_back(j.rpy[i]);
        for (int i = 0; i < 3; i++) axis.push_back(j.axis[i]);
        float g = 0.0f;
        if (use_torque_adjustment_) {
          const auto it = std::find(adjustment_joints_.begin(), adjustment_joints_.end(), j.name);
          if (it != adjustment_joints_.end()) g = adjustment_gain_[(size_t) (it - adjustment_joints_.begin())];
        }
        gain.push_back(g);
      }
    if (use_torque_adjustment_)
      for (const std::string &n : adjustment_joints_)
        if (std::find(msg->joint_name.begin(), msg->joint_name.end(), n) == msg->joint_name.end()) {
          fprintf(stdout, "TorqueAdjustment: %s joint not found\n", n.c_str());  // torque_adjustment.cpp:44-46
          exit(-1);
        }
    if (pb_legodo_set_chain(est->ctx, (int) model_->left_chain.size(), (int) model_->right_chain.size(), type.data(), row.data(), org.data(),
                            axis.data(), use_torque_adjustment_ ? gain.data() : nullptr) != PB_OK)
      pb_report_exit("LegOdoHandler", est->ctx);
    if (filter_joint_positions_ != 0) {
      // SimpleKalmanFilter(joint_process_noise, joint_observation_noise) (leg_estimate.cpp:56): the two values land in
      // process_noise_pos_ and process_noise_vel_, observation_noise_ keeps its default 5E-4 (simple_kalman_filter.hpp:15).
      // A new joint order (a new chain) starts the filters over.
      if (pb_joint_filter_init(est->ctx, filter_joint_positions_, joint_process_noise_, joint_observation_noise_, 5E-4) != PB_OK)
        pb_report_exit("LegOdoHandler", est->ctx);
      // per-filter joint states: the filtered block [rows][B] and, for host messages, the two foot forces [2][B] behind it
      jf_pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(float) * (msg->joint_name.size() + 2) * (size_t) est->B);
    }
    chain_names_ = msg->joint_name;
    chain_ready_ = true;
  }

  // one message's leg inputs, kept alive by the update made from them: broadcast values are copied (they are a few dozen
  // numbers), device arrays are referenced (the caller keeps them, as everywhere), host blocks are used before the handler
  // returns
  struct LegMsg {
    int kind = 0, mem = PB_HOST, rows = 0;       // kind 0: foot poses, 1: joint state
    int64_t utime = 0;
    const float *jp = nullptr, *je = nullptr, *ff = nullptr;
    const double *feet = nullptr, *forces = nullptr;
    std::vector<float> own_f;
    std::vector<double> own_d;
    std::shared_ptr<DeviceBlock> filtered;   // the joint filters' output block, when they run on the device
    std::shared_ptr<DeviceBlock> forces_dev; // the foot forces of a host force/torque message uploaded next to a device joint block
    std::vector<int64_t> own_ut;             // per-filter message times / validity (independent log segments), copied: the odometry
    std::vector<uint8_t> own_valid;          // may run after the handler has returned
    const int64_t *dev_ut = nullptr;         // ... or device arrays, referenced like every PB_DEVICE input (valid until the update
    const uint8_t *dev_valid = nullptr;      // made from this message has been applied)
    double r = 0, ru = 0;
    int times(pb_ctx *ctx) const
    {
      if (dev_ut != nullptr || dev_valid != nullptr) return pb_legodo_set_message_times(ctx, dev_ut, dev_valid, PB_DEVICE);
      if (own_ut.empty() && own_valid.empty()) return PB_OK;
      return pb_legodo_set_message_times(ctx, own_ut.empty() ? nullptr : own_ut.data(), own_valid.empty() ? nullptr : own_valid.data(), PB_HOST);
    }
    // odometry alone (imu == NULL) or slaved to the state after `imu`; outputs as pb_legodo_update_joints
    int odometry(pb_ctx *ctx, const BatchArray *imu, double *o_delta, double *o_status, double *d_lo, uint8_t *d_mask, double *o_pos,
                 uint8_t *o_pos_ok) const
    {
      const int trc = times(ctx);
      if (trc != PB_OK) return trc;
      if (kind == 1)
        return pb_legodo_update_joints(ctx, imu ? imu->p : nullptr, imu ? imu->mem : PB_DEVICE, utime, rows, jp, je, ff, mem, 0, r, ru, o_delta,
                                       o_status, d_lo, d_mask, o_pos, o_pos_ok);
      return imu ? pb_legodo_update_after_predict(ctx, imu->p, imu->mem, utime, feet, forces, mem, 0, r, ru, o_delta, o_status, d_lo, d_mask)
                 : pb_legodo_update(ctx, utime, feet, forces, mem, 0, r, ru, o_delta, o_status, d_lo, d_mask);
    }
    // INS step + odometry + update in one call (one kernel where the library has it)
    int pair(pb_ctx *ctx, const RBISIMUProcessStep *imu, double *d_lo, uint8_t *d_mask) const
    {
      const double q[4] = { imu->q_gyro, imu->q_accel, imu->q_gyro_bias, imu->q_accel_bias };
      const int trc = times(ctx);
      if (trc != PB_OK) return trc;
      imu->announce(ctx);
      if (kind == 1)
        return pb_step_legodo_joints(ctx, imu->imu_block.p, imu->imu_block.mem, q, utime, rows, jp, je, ff, mem, r, ru, d_lo, d_mask);
      return pb_step_legodo_feet(ctx, imu->imu_block.p, imu->imu_block.mem, q, utime, feet, forces, mem, r, ru, d_lo, d_mask);
    }
  };

  // the measurement of `u` is still to be made from `lm`, into d_lo / d_mask: inside the pair kernel, or on its own (RBISIndexedMeasurement)
  static void deferTo(RBISIndexedMeasurement *u, const std::shared_ptr<LegMsg> &lm, double *d_lo, uint8_t *d_mask)
  {
    u->pair_kernel = [lm, d_lo, d_mask](pb_ctx *ctx, const RBISIMUProcessStep *imu, bool keep) {
      return lm->pair(ctx, imu, keep ? d_lo : nullptr, keep ? d_mask : nullptr);
    };
    u->make_measurement = [lm, d_lo, d_mask](pb_ctx *ctx, const RBISIMUProcessStep *ahead_of) {
      return lm->odometry(ctx, ahead_of ? &ahead_of->imu_block : nullptr, nullptr, nullptr, d_lo, d_mask, nullptr, nullptr);
    };
  }
  // what the device-side entry points share: the pending-IMU decision, the odometry and the measurement LegOdoCommon forms
  // from its result
  RBISUpdateInterface *odometryUpdate(MavStateEstimator *est, std::shared_ptr<LegMsg> lm)
  {
    const int B = est->B;
    const int64_t utime = lm->utime;
    const LegOdoCommon *lc = leg_odo_common_;
    lm->r = lc->R_legodo_vxyz_;
    lm->ru = lc->R_legodo_vxyz_uncertain_;
    // The odometry reads the head pose.  An INS step that fuse_ins_legodo is holding back is either applied first, or -- when
    // the measurement made here will pair with it -- left pending: the pair then runs as ONE kernel that does the INS step, the
    // odometry slaved to the pose after it and the update in LegOdoCommon's mode (pb_step_legodo_joints / _feet).
    RBISIMUProcessStep *ahead = est->pendingImu();
    if (ahead != nullptr && ahead->imu_block.mem == PB_HOST && lm->mem == PB_HOST) ahead = nullptr;  // one host staging area
    if (ahead == nullptr) est->flushPending();
    if (!legodo_ready_) initLegEstimate(est);
    if (sweep_dirty_) applySweep(est);
    if (control_contacts_dirty_) {
      if (pb_legodo_set_control_contacts(est->ctx, n_control_contacts_, PB_HOST_BROADCAST) != PB_OK) pb_report("LegOdoHandler", est->ctx);
      control_contacts_dirty_ = false;
    }
    const std::shared_ptr<DeviceBlock> block = take_block(pool_);
    if (!block) return pb_report("LegOdoHandler", est->ctx);
    double *d_lo = (double *) block->p;
    uint8_t *d_mask = (uint8_t *) (d_lo + (size_t) 6 * B);   // lin_rate: z [3][B] | R diagonal [3][B] | mask [B]
    // LegOdoCommon::createMeasurement runs on the DEVICE for every mode (pb_legodo_set_measurement_mode): the increment, the status
    // and the position never cross PCIe.  A foot-state message has no pelvis position: mode pos_and_lin_rate then is the
    // reference's own fall-back to lin_rate (rbis_legodo_common.cpp:118-122) for every filter.
    const int dmode = (lc->mode_ == LegOdoCommon::MODE_LIN_AND_ROT_RATE) ? 1 : ((lc->mode_ == LegOdoCommon::MODE_POSITION_AND_LIN_RATE && lm->kind == 1) ? 2 : 0);
    if (dmode != device_meas_mode_) {
      if (pb_legodo_set_measurement_mode(est->ctx, dmode, lc->R_legodo_xyz_, lc->R_legodo_vang_, lc->R_legodo_vang_uncertain_) != PB_OK)
        return pb_report("LegOdoHandler", est->ctx);
      device_meas_mode_ = dmode;
    }
    const bool lin = dmode == 0;
    if (!lin) d_mask = (uint8_t *) (d_lo + (size_t) 12 * B);   // z [6][B] | R diagonal [6][B] | masks [2][B]
    // the measurement can be made later, inside the step kernel, when its inputs outlive this call
    const bool defer = ahead != nullptr && one_kernel_pairs && lm->mem != PB_HOST;
    if (!defer) {
      if (lm->odometry(est->ctx, ahead ? &ahead->imu_block : nullptr, nullptr, nullptr, d_lo, d_mask, nullptr, nullptr) != PB_OK)
        return pb_report("LegOdoHandler", est->ctx);
    }
    prev_legodo_utime_ = utime;
    std::vector<int> idx = RBIS::velocityInds();   // lin_rate: three rows
    if (!lin) {
      double unused[6];
      lc->getCovariance(lc->mode_, true, unused, &idx);   // (assigns idx: the six rows of the mode)
    }
    // the block is z [m][B], then the diagonal of R [m][B], m = 3 or 6
    auto *full = new RBISIndexedMeasurement(idx, BatchArray(d_lo, PB_DEVICE), d_lo + idx.size() * B, PB_R_DIAG, d_mask, RBISUpdateInterface::legodo, utime);
    full->owned_dev = block;
    if (defer) deferTo(full, lm, d_lo, d_mask);  // (the block holds the rows and masks of BOTH halves of mode 2's either-update)
    if (dmode != 2) return full;
    // pos_and_lin_rate: the filters whose position is not valid take the lin_rate update on the velocity rows of the same block
    auto *fallback = new RBISIndexedMeasurement(RBIS::velocityInds(), BatchArray(d_lo + (size_t) 3 * B, PB_DEVICE), d_lo + (size_t) 9 * B, PB_R_DIAG,
                                                d_mask + (size_t) B, RBISUpdateInterface::legodo, utime);
    fallback->owned_dev = block;
    return new RBISEitherUpdate(full, fallback);
  }
  int device_meas_mode_ = 0;
  int64_t prev_legodo_utime_ = 0;
  // false: always make the measurement in the handler (k_legodo), then the fused step reads it -- round 2's two launches
  bool one_kernel_pairs = true;

  // the reference's handler (rbis_legodo_update.cpp:206-280)
  RBISUpdateInterface *processMessage(const msgs::joint_state_t *msg, MavStateEstimator *est)
  {
    if (!forceTorqueSeen()) return nullptr;
    if (model_ == nullptr) {
      fprintf(stderr, "LegOdoHandler: a joint_state_t needs the robot model (construct the handler with a ModelClient)\n");
      exit(1);
    }
    if (!legodo_ready_) initLegEstimate(est);
    if (sweep_dirty_) applySweep(est);
    if (!chain_ready_ || msg->joint_name != chain_names_) initChain(msg, est);
    const float *forces = foot_force_dev_ ? foot_force_dev_ : foot_force_.data();
    int fmem = foot_force_dev_ ? PB_DEVICE : foot_force_mem_;
    auto lm = std::make_shared<LegMsg>();
    if (fmem == PB_HOST && msg->mem == PB_DEVICE) {
      // a device-resident joint block with the force/torque message still on the host (SegmentBatcher uploads the big blocks
      // itself): the 2 x B floats follow the joints into HBM, in a block this message owns
      if (!ff_pool_) ff_pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(float) * 2 * (size_t) est->B);
      bool fresh = false;
      void *blk = ff_pool_->get(fresh);
      if (blk == nullptr || pb_memcpy_h2d(est->ctx, blk, forces, sizeof(float) * 2 * (size_t) est->B) != PB_OK) return pb_report("LegOdoHandler", est->ctx);
      lm->forces_dev = std::make_shared<DeviceBlock>(ff_pool_, blk);
      forces = (const float *) blk;
      fmem = PB_DEVICE;
    }
    if (fmem != msg->mem) {
      fprintf(stderr, "LegOdoHandler: the joint state and the force/torque message must live in the same memory space\n");
      return nullptr;
    }
    lm->kind = 1;
    lm->mem = msg->mem;
    lm->rows = (int) msg->joint_name.size();
    lm->utime = msg->utime;
    if (msg->times_mem == PB_DEVICE) {
      lm->dev_ut = msg->utimes;
      lm->dev_valid = msg->valid;
    } else {
      if (msg->utimes != nullptr) lm->own_ut.assign(msg->utimes, msg->utimes + est->B);
      if (msg->valid != nullptr) lm->own_valid.assign(msg->valid, msg->valid + est->B);
    }
    if (msg->utimes != nullptr && filter_joint_positions_ == 2) {
      fprintf(stderr, "LegOdoHandler: per-filter message times with filter_joint_positions = kalman are not supported (the joint Kalman filters keep one clock per batch)\n");
      return nullptr;
    }
    const float *eff = use_torque_adjustment_ ? msg->joint_effort : nullptr;
    if (filter_joint_positions_ != 0) {
      // leg_estimate.cpp:411-428, after the torque adjustment (rbis_legodo_update.cpp:231-241): pb_joint_filter does both, the
      // kinematics then read the filtered block without an effort
      if (filter_joint_positions_ == 2 && msg->joint_velocity == nullptr) {
        fprintf(stderr, "LegOdoHandler: filter_joint_positions = kalman reads joint_velocity\n");
        return nullptr;
      }
      float *out = nullptr;
      if (msg->mem == PB_HOST_BROADCAST) {
        lm->own_f.assign((size_t) lm->rows + 2, 0.0f);
        out = lm->own_f.data();
      } else {
        lm->filtered = take_block(jf_pool_);
        if (!lm->filtered) return pb_report("LegOdoHandler", est->ctx);
        out = (float *) lm->filtered->p;
      }
      if (pb_joint_filter(est->ctx, msg->utime, lm->rows, msg->joint_position, msg->joint_velocity, eff, msg->mem, out) != PB_OK)
        return pb_report("LegOdoHandler", est->ctx);
      lm->jp = out;
      lm->je = nullptr;
      if (msg->mem == PB_HOST_BROADCAST) {
        lm->own_f[(size_t) lm->rows] = forces[0];
        lm->own_f[(size_t) lm->rows + 1] = forces[1];
        lm->ff = lm->own_f.data() + lm->rows;
      } else {
        lm->ff = forces;
        if (msg->mem == PB_HOST) {  // the filtered joints are in HBM: the foot forces of a host message follow them there
          float *dff = out + (size_t) lm->rows * est->B;
          if (pb_memcpy_h2d(est->ctx, dff, forces, sizeof(float) * 2 * (size_t) est->B) != PB_OK) return pb_report("LegOdoHandler", est->ctx);
          lm->ff = dff;
          lm->mem = PB_DEVICE;
        }
      }
    } else if (msg->mem == PB_HOST_BROADCAST) {  // one robot's message: own the few numbers
      lm->own_f.assign(msg->joint_position, msg->joint_position + lm->rows);
      if (eff) lm->own_f.insert(lm->own_f.end(), eff, eff + lm->rows);
      lm->own_f.insert(lm->own_f.end(), forces, forces + 2);
      lm->jp = lm->own_f.data();
      lm->je = eff ? lm->own_f.data() + lm->rows : nullptr;
      lm->ff = lm->own_f.data() + (eff ? 2 : 1) * (size_t) lm->rows;
    } else {
      lm->jp = msg->joint_position;
      lm->je = eff;
      lm->ff = forces;
    }
    return odometryUpdate(est, lm);
  }

  // the same from what forward kinematics produces (msgs::foot_state_t); no pelvis position: mode pos_and_lin_rate falls back
  // to lin_rate like the reference does while its world constraint is not initialised (rbis_legodo_common.cpp:118-122)
  RBISUpdateInterface *processMessageFeet(const msgs::foot_state_t *msg, MavStateEstimator *est)
  {
    if (!forceTorqueSeen()) return nullptr;
    auto lm = std::make_shared<LegMsg>();
    lm->kind = 0;
    lm->mem = msg->feet.mem;
    lm->utime = msg->utime;
    if (msg->feet.mem == PB_HOST_BROADCAST) {
      lm->own_d.assign(msg->feet.p, msg->feet.p + 14);
      lm->own_d.insert(lm->own_d.end(), msg->forces.p, msg->forces.p + 2);
      lm->feet = lm->own_d.data();
      lm->forces = lm->own_d.data() + 14;
    } else {
      lm->feet = msg->feet.p;
      lm->forces = msg->forces.p;
    }
    return odometryUpdate(est, lm);
  }

  // from a finished increment (a caller that runs its own leg_estimate): createMeasurement and the handler's gates
  RBISUpdateInterface *processMessageDelta(const msgs::legodo_delta_t *msg, MavStateEstimator *est)
  {
    if (!forceTorqueSeen()) return nullptr;
    // (:243-255) "Leg Odometry is not valid not integrating": no update and no decrement when no filter has a valid increment
    if (msg->delta_status != nullptr) {
      bool any = false;
      for (int b = 0; b < est->B && !any; b++) any = msg->delta_status[b] >= 0;
      if (!any) return nullptr;
    }
    // "Ignore the calculated velocity at launch" (:264-269): decrement FIRST, then compare -- N zeroes N-1 ticks
    zero_initial_velocity--;
    if (zero_initial_velocity > 0) {
      std::vector<double> zero((size_t) 3 * est->B, 0.0);
      msgs::legodo_delta_t m2 = *msg;
      m2.delta_trans = zero.data();   // odo_delta.setIdentity()
      m2.delta_quat = nullptr;
      if (msg->position != nullptr) m2.position = zero.data();  // odo_position.setIdentity(), status passed on as is
      return leg_odo_common_->createMeasurement(&m2, est->B);
    }
    return leg_odo_common_->createMeasurement(msg, est->B);
  }
};

// The reference's update objects own their measurement (Eigen copies in their constructors); so do ours for host data,
// which the history may re-apply long after the message buffer is gone.  Device blocks are referenced, not copied: the
// caller keeps them alive for utime_history_span.  cov_diag must outlive the update (handlers are app-lifetime singletons).
// ---------------------------------------------------------------------------------------------------------------
// YawLockHandler (motion_estimate/src/quick_lock/rbis_yawlock_update.cpp): the reference's constructor (lcm_recv, lcm_pub, param,
// model, frames) without the LCM objects; `ins_to_body` is what it takes from BotFrames (:45-47).  The caller routes the status
// channel named by behavior_channel to controllerStatusHandler / robotBehaviorHandler and the IMU channel to insHandler, and adds
// processMessage as sensor "yawlock" (FrontEnd::addSensor) behind the LegOdoHandler of the same joint-state channel
// (fusion.cpp:233-241 registers legodo first): the kinematic chain on the device is the one that handler sets.
// The state machine itself (YawLock::getCorrection) lives per filter on the device, rbis_yawlock.hpp.
// ---------------------------------------------------------------------------------------------------------------
class YawLockHandler {
public:
  enum YawLockMode { MODE_YAWBIAS = 0, MODE_YAW = 1, MODE_YAWBIAS_YAW = 2 };
  YawLockMode mode;
  int correction_period;
  bool yaw_slip_detect;
  double yaw_slip_threshold_degrees, yaw_slip_disable_period, r_yaw_bias = 0.0, r_yaw = 0.0;
  std::string behavior_channel, left_standing_link, right_standing_link;
  BotTrans ins_to_body;
  double body_gyro[3] = { 0, 0, 0 };
  bool is_robot_standing = false;        // yaw_lock_->setIsRobotStanding (yawlock.cpp:60: false at the start)
  int64_t last_ihmc_walking_utime = 0;   // rbis_yawlock_update.cpp:107
  int64_t idle_messages = 0;             // messages whose update reached no filter (the reference's NULL return), counted lazily

  YawLockHandler(BotParam *param, const ModelClient *model, const BotTrans *ins_to_body_ = nullptr) : model_(model)
  {
    correction_period = (int) bot_param_get_int_or_fail(param, "state_estimator.yawlock.correction_period");
    yaw_slip_detect = bot_param_get_boolean_or_fail(param, "state_estimator.yawlock.yaw_slip_detect");
    yaw_slip_threshold_degrees = bot_param_get_double_or_fail(param, "state_estimator.yawlock.yaw_slip_threshold_degrees");
    // NB the reference reads yaw_slip_disable_period from the key yaw_slip_threshold_degrees (rbis_yawlock_update.cpp:19):
    // mirrored as it is, a threshold of 1.5 degrees is also a hold-off of 1.5 seconds
    yaw_slip_disable_period = bot_param_get_double_or_fail(param, "state_estimator.yawlock.yaw_slip_threshold_degrees");
    behavior_channel = bot_param_get_str_or_fail(param, "state_estimator.yawlock.behavior_channel");
    left_standing_link = bot_param_get_str_or_fail(param, "state_estimator.legodo.left_standing_link");
    right_standing_link = bot_param_get_str_or_fail(param, "state_estimator.legodo.right_standing_link");
    if (behavior_channel != "CONTROLLER_STATUS" && behavior_channel != "ROBOT_BEHAVIOR") {  // :30-41
      fprintf(stdout, "behavior_channel not recognised: CONTROLLER_STATUS or ROBOT_BEHAVIOR\n");
      exit(-1);
    }
    if (ins_to_body_) ins_to_body = *ins_to_body_;
    const std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.yawlock.mode");
    if (mode_str == "yawbias") mode = MODE_YAWBIAS;
    else if (mode_str == "yaw") mode = MODE_YAW;
    else if (mode_str == "yawbias_yaw") mode = MODE_YAWBIAS_YAW;
    else {  // :66-69
      mode = MODE_YAW;
      fprintf(stdout, "Unrecognized scan matcher mode. Will reject yaw drift by default.\n");
    }
    if (mode != MODE_YAW) r_yaw_bias = bot_param_get_double_or_fail(param, "state_estimator.yawlock.r_yaw_bias");  // :79, :93 deg per sec
    if (mode != MODE_YAWBIAS) r_yaw = bot_param_get_double_or_fail(param, "state_estimator.yawlock.r_yaw");       // :87, :94
  }

  // rbis_yawlock_update.cpp:112-116: the gyro in the body frame
  void insHandler(const msgs::ins_t *msg)
  {
    // (one robot's message, PB_HOST_BROADCAST, or filter 0's sample of a per-filter HOST block: the handler keeps one value)
    const double g[3] = { msg->gyro.p[0], msg->gyro.mem == PB_HOST_BROADCAST ? msg->gyro.p[1] : msg->gyro.p[(size_t) gyro_stride_],
                          msg->gyro.mem == PB_HOST_BROADCAST ? msg->gyro.p[2] : msg->gyro.p[2 * (size_t) gyro_stride_] };
    bot_quat_rotate_to(ins_to_body.rot_quat, g, body_gyro);
  }
  // MIT / Drake status (:125-137)
  void controllerStatusHandler(const msgs::controller_status_t *msg)
  {
    is_robot_standing = msg->state == msgs::controller_status_t::STANDING || msg->state == msgs::controller_status_t::MANIPULATING;
  }
  // IHMC status (:140-158)
  void robotBehaviorHandler(const msgs::behavior_t *msg)
  {
    bool standing = msg->behavior == msgs::behavior_t::BEHAVIOR_STAND || msg->behavior == msgs::behavior_t::BEHAVIOR_MANIPULATE;
    // "IHMC's behavior message is faulty: it reports the robot standing when it is finishing the last few seconds of a walking
    // plan" (rbis_yawlock_update.cpp:146-154): less than 3 s after the last BEHAVIOR_WALK counts as not standing
    if (msg->behavior == msgs::behavior_t::BEHAVIOR_WALK) last_ihmc_walking_utime = msg->utime;
    if (msg->utime - last_ihmc_walking_utime < 3E6) standing = false;
    is_robot_standing = standing;
  }

  // rbis_yawlock_update.cpp:168-232.  Never NULL for the batch: which filters get which row set is decided per filter on the
  // device when the update is applied; a message that reaches no filter is an update with two empty masks
  // (RBISUpdateInterface::appliesToNoFilter), as LegOdoHandler's per-filter NULL returns are.
  RBISUpdateInterface *processMessage(const msgs::joint_state_t *msg, MavStateEstimator *est)
  {
    if (!ready_) {
      if (pb_yawlock_init(est->ctx, (int) mode, correction_period, yaw_slip_detect, yaw_slip_threshold_degrees, yaw_slip_disable_period,
                          r_yaw_bias, r_yaw) != PB_OK)
        pb_report_exit("YawLockHandler", est->ctx);
      pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, (sizeof(double) * 6 + 2) * (size_t) est->B);
      gyro_stride_ = est->B;
      ready_ = true;
    }
    if (msg->mem == PB_HOST) {
      fprintf(stderr, "YawLockHandler: joint positions must be PB_HOST_BROADCAST (one robot) or PB_DEVICE blocks\n");
      return nullptr;
    }
    std::shared_ptr<DeviceBlock> block = take_block(pool_);
    if (!block) return nullptr;
    const msgs_joint_ref j{ msg->joint_position, (int) msg->joint_name.size(), msg->mem };
    return new RBISYawLockUpdate((int) mode, j, is_robot_standing ? 1 : 0, body_gyro[2], bot_sq(bot_to_radians(r_yaw_bias)),
                                 bot_sq(bot_to_radians(r_yaw)), std::move(block), msg->utime);
  }

private:
  const ModelClient *model_;
  std::shared_ptr<DevicePool> pool_;
  int gyro_stride_ = 1;
  bool ready_ = false;
};

inline RBISIndexedMeasurement *makeIndexedMeasurement(const std::vector<int> &idx, BatchArray z, int B,
                                                      const std::vector<double> &cov_diag, const uint8_t *mask,
                                                      RBISUpdateInterface::sensor_enum sensor, int64_t utime)
{
  if (z.mem == PB_DEVICE) return new RBISIndexedMeasurement(idx, z, cov_diag.data(), PB_R_DIAG_BROADCAST, mask, sensor, utime);
  return hostIndexedMeasurement(idx, own_rows(z, idx.size(), B), cov_diag, PB_R_DIAG_BROADCAST, own_mask(mask, z.mem, B), z.mem, sensor, utime);
}

// What the processMessageInit of a pose sensor does to the state it initialises: the position rows and their covariance block
// diag(cov_xyz) from pos [3][B] and, with `quat` [4][B], the quaternion and the chi block r_chi2 * I.  Host (or host-broadcast) arrays.
// Filters with only[b] == 0 keep what they have; returns whether any filter was initialised.
inline bool initPositionOrientation(RBIS &init_state, RBIM &init_cov, BatchArray pos, const double cov_xyz[3], const uint8_t *only = nullptr,
                                    const double *quat = nullptr, double r_chi2 = 0.0)
{
  const int B = init_state.B;
  const size_t per = batch_per(pos.mem, B);
  bool any = false;
  for (int b = 0; b < B; b++) {
    if (only != nullptr && !only[b]) continue;
    any = true;
    const size_t sb = (per == 1) ? 0 : (size_t) b;
    for (int i = 0; i < 3; i++) {
      init_state(RBIS::position_ind + i, b) = pos.p[(size_t) i * per + sb];
      for (int j = 0; j < 3; j++) {
        init_cov(RBIS::position_ind + i, RBIS::position_ind + j, b) = (i == j) ? cov_xyz[i] : 0.0;
        if (quat != nullptr) init_cov(RBIS::chi_ind + i, RBIS::chi_ind + j, b) = (i == j) ? r_chi2 : 0.0;
      }
    }
    for (int i = 0; quat != nullptr && i < 4; i++) init_state.q(i, b) = quat[(size_t) i * per + sb];
  }
  return any;
}

class ScanMatcherHandler {
public:
  typedef enum { MODE_POSITION, MODE_POSITION_YAW, MODE_VELOCITY, MODE_VELOCITY_YAW, MODE_YAW } ScanMatchingMode;
  ScanMatchingMode mode;
  std::vector<int> z_indices;
  std::vector<double> cov_scan_match;  // diagonal

  explicit ScanMatcherHandler(BotParam *param)
  {
    std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.scan_matcher.mode");
    if (mode_str == "position") mode = MODE_POSITION;
    else if (mode_str == "position_yaw") mode = MODE_POSITION_YAW;
    else if (mode_str == "velocity") mode = MODE_VELOCITY;
    else if (mode_str == "velocity_yaw") mode = MODE_VELOCITY_YAW;
    else if (mode_str == "yaw") mode = MODE_YAW;
    else mode = MODE_VELOCITY;  // sensor_handlers.cpp:636-639
    if (mode == MODE_POSITION || mode == MODE_POSITION_YAW) {
      double rxy = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_pxy");
      double rz = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_pz");
      cov_scan_match = { bot_sq(rxy), bot_sq(rxy), bot_sq(rz) };
      z_indices = RBIS::positionInds();
    } else if (mode == MODE_YAW) {
      double ry = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_yaw");
      cov_scan_match = { bot_sq(bot_to_radians(ry)) };
      z_indices = { RBIS::chi_ind + 2 };
    } else {
      double rxy = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_vxy");
      double rz = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_vz");
      cov_scan_match = { bot_sq(rxy), bot_sq(rxy), bot_sq(rz) };
      z_indices = RBIS::velocityInds();
    }
    if (mode == MODE_POSITION_YAW || mode == MODE_VELOCITY_YAW) {
      double ry = bot_param_get_double_or_fail(param, "state_estimator.scan_matcher.r_yaw");
      cov_scan_match.push_back(bot_sq(bot_to_radians(ry)));
      z_indices.push_back(RBIS::chi_ind + 2);
    }
  }

  // sensor_handlers.cpp:689-724.  For the *_yaw modes z is [4][B] whose 4th row is ignored (chi index), so the
  // message's pos/vel block is used in place when it already has 4 rows of storage; otherwise it is padded on the host.
  RBISUpdateInterface *processMessage(const msgs::pose_t *msg, MavStateEstimator *est)
  {
    const int B = est->B;
    if (mode == MODE_POSITION)
      return makeIndexedMeasurement(RBIS::positionInds(), msg->pos, B, cov_scan_match, msg->valid, RBISUpdateInterface::scan_matcher,
                                    msg->utime);
    if (mode == MODE_VELOCITY)
      return makeIndexedMeasurement(RBIS::velocityInds(), msg->vel, B, cov_scan_match, msg->valid, RBISUpdateInterface::scan_matcher,
                                    msg->utime);
    const BatchArray src = (mode == MODE_POSITION_YAW) ? msg->pos : msg->vel;
    const int m = (int) z_indices.size();
    const int omem = msg->orientation.mem;
    if (omem == PB_DEVICE || (mode != MODE_YAW && src.mem != omem)) {
      fprintf(stderr, "ScanMatcherHandler: *_yaw modes take host (or host-broadcast) pos/vel and orientation arrays\n");
      return nullptr;
    }
    const size_t per = batch_per(omem, B);
    std::vector<double> z((size_t) m * per, 0.0);
    if (mode != MODE_YAW) memcpy(z.data(), src.p, sizeof(double) * 3 * per);
    return hostIndexedPlusOrientationMeasurement(z_indices, std::move(z), cov_scan_match, own_rows(msg->orientation, 4, B), own_mask(msg->valid, omem, B), omem,
                                                 RBISUpdateInterface::scan_matcher, msg->utime);
  }
};

class IndexedMeasurementHandler {
public:
  explicit IndexedMeasurementHandler(RBISUpdateInterface::sensor_enum this_sensor) : indexed_sensor(this_sensor) {}
  RBISUpdateInterface *processMessage(const msgs::indexed_measurement_t *msg, MavStateEstimator *est)
  {
    // sensor_handlers.cpp:576-582.  Like the reference's update object, ours owns a copy of host data (it may be
    // re-applied later from the history); device blocks stay where they are.
    const int m = (int) msg->z_indices.size();
    if (msg->z_effective.mem == PB_DEVICE)
      return new RBISIndexedMeasurement(msg->z_indices, msg->z_effective, msg->R_effective, PB_R_FULL, nullptr, indexed_sensor,
                                        msg->utime);
    const int mem = msg->z_effective.mem, B = est ? est->B : 1;   // (a host-only caller hands one robot's message over without an estimator)
    return hostIndexedMeasurement(msg->z_indices, own_rows(msg->z_effective, (size_t) m, B), own_rows(BatchArray(msg->R_effective, mem), (size_t) m * m, B),
                                  PB_R_FULL, {}, mem, indexed_sensor, msg->utime);
  }
  // processMessageInit (sensor_handlers.cpp:584-610): the measured entries and their covariance block initialise the
  // state; chi entries are folded into the quaternion (init_state.chiToQuat()).  Host messages only.
  double chi_tol = 1e-6;  // eigen_utils' chiToQuat tolerance (the same constant as pb_set_constants' chi_tol)
  bool processMessageInit(const msgs::indexed_measurement_t *msg, const std::map<std::string, bool> & /*sensors_initialized*/,
                          const RBIS & /*default_state*/, const RBIM & /*default_cov*/, RBIS &init_state, RBIM &init_cov)
  {
    if (msg->z_effective.mem == PB_DEVICE) return false;
    const int B = init_state.B, m = (int) msg->z_indices.size();
    const size_t per = batch_per(msg->z_effective.mem, B);
    for (int b = 0; b < B; b++) {
      const size_t sb = (per == 1) ? 0 : (size_t) b;
      for (int ii = 0; ii < m; ii++) {
        if (msg->z_indices[(size_t) ii] >= init_state.n) continue;  // a 15-state batch has no bias entries to initialise
        for (int jj = 0; jj < m; jj++)
          if (msg->z_indices[(size_t) jj] < init_state.n)
            init_cov(msg->z_indices[(size_t) ii], msg->z_indices[(size_t) jj], b) = msg->R_effective[(size_t) (jj * m + ii) * per + sb];
        init_state(msg->z_indices[(size_t) ii], b) = msg->z_effective.p[(size_t) ii * per + sb];
      }
      // chiToQuat: quat <- quat * Exp(chi), chi <- 0, when |chi| exceeds the tolerance
      const double c[3] = { init_state(6, b), init_state(7, b), init_state(8, b) };
      const double ang = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
      if (ang > chi_tol) {
        const double sh = sin(0.5 * ang) / ang, dq[4] = { cos(0.5 * ang), c[0] * sh, c[1] * sh, c[2] * sh };
        const double q0[4] = { init_state.q(0, b), init_state.q(1, b), init_state.q(2, b), init_state.q(3, b) };
        double qn[4];
        quat_mult(q0, dq, qn);
        for (int i = 0; i < 4; i++) init_state.q(i, b) = qn[i];
        init_state(6, b) = init_state(7, b) = init_state(8, b) = 0.0;
      }
    }
    return true;
  }
private:
  RBISUpdateInterface::sensor_enum indexed_sensor;
};

class GpsHandler {
public:
  std::vector<double> cov_xyz;  // diagonal
  explicit GpsHandler(BotParam *_param)
  {
    double rxy = bot_param_get_double_or_fail(_param, "state_estimator.gps.r_xy");
    double rz = bot_param_get_double_or_fail(_param, "state_estimator.gps.r_z");
    cov_xyz = { rxy * rxy, rxy * rxy, rz * rz };
  }
  RBISUpdateInterface *processMessage(const msgs::gps_data_t *msg, MavStateEstimator *est)
  {
    return makeIndexedMeasurement(RBIS::positionInds(), msg->xyz_pos, est->B, cov_xyz, msg->has_lock, RBISUpdateInterface::gps,
                                  msg->utime);  // sensor_handlers.cpp:374-381
  }
  // processMessageInit (sensor_handlers.cpp:383-403): position and its covariance from the fix (filters without lock keep theirs)
  bool processMessageInit(const msgs::gps_data_t *msg, const std::map<std::string, bool> & /*sensors_initialized*/,
                          const RBIS & /*default_state*/, const RBIM & /*default_cov*/, RBIS &init_state, RBIM &init_cov)
  {
    if (msg->xyz_pos.mem == PB_DEVICE) return false;
    init_state.utime = msg->utime;
    return initPositionOrientation(init_state, init_cov, msg->xyz_pos, cov_xyz.data(), msg->has_lock);
  }
};

// ViconHandler (sensor_handlers.cpp:406-574): motion-capture pose as position / orientation / yaw / position+orientation
// measurement.  local_to_body = local_to_vicon o body_to_vicon when apply_frame (libbot's bot_trans_apply_trans_to
// [NOT IN TREE]: rotation q1 * q2, translation R(q1) t2 + t1).  Host (or host-broadcast) messages.
class ViconHandler {
public:
  typedef enum { MODE_POSITION, MODE_POSITION_ORIENT, MODE_ORIENTATION, MODE_YAW } ViconMode;
  ViconMode mode;
  bool apply_frame;
  BotTrans body_to_vicon;
  std::vector<int> z_indices;
  std::vector<double> cov_vicon;  // diagonal, of the measured entries
  double r_xyz2, r_chi2;
  ViconHandler(BotParam *param, const BotTrans *body_to_vicon_ = nullptr)
  {
    const std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.vicon.mode");
    if (mode_str == "position") mode = MODE_POSITION;
    else if (mode_str == "position_orient") mode = MODE_POSITION_ORIENT;
    else if (mode_str == "orientation") mode = MODE_ORIENTATION;
    else if (mode_str == "yaw") mode = MODE_YAW;
    else {
      mode = MODE_POSITION;
      fprintf(stdout, "Unrecognized Vicon mode. Using position mode by default.\n");
    }
    apply_frame = bot_param_get_boolean_or_fail(param, "state_estimator.vicon.apply_frame");
    if (apply_frame && body_to_vicon_) body_to_vicon = *body_to_vicon_;
    r_xyz2 = bot_sq(bot_param_get_double_or_fail(param, "state_estimator.vicon.r_xyz"));
    r_chi2 = bot_sq(bot_to_radians(bot_param_get_double_or_fail(param, "state_estimator.vicon.r_chi")));
    if (mode == MODE_POSITION) { z_indices = RBIS::positionInds(); cov_vicon = { r_xyz2, r_xyz2, r_xyz2 }; }
    else if (mode == MODE_YAW) { z_indices = { RBIS::chi_ind + 2 }; cov_vicon = { r_chi2 }; }
    else if (mode == MODE_ORIENTATION) { z_indices = RBIS::chiInds(); cov_vicon = { r_chi2, r_chi2, r_chi2 }; }
    else { z_indices = { 9, 10, 11, 6, 7, 8 }; cov_vicon = { r_xyz2, r_xyz2, r_xyz2, r_chi2, r_chi2, r_chi2 }; }
  }
  RBISUpdateInterface *processMessage(const msgs::rigid_transform_t *msg, MavStateEstimator *est)
  {
    std::vector<double> t, q;
    std::vector<uint8_t> mask;
    int mem;
    if (!to_body(msg, est->B, t, q, mask, mem)) return nullptr;
    const int m = (int) z_indices.size();
    const size_t per = t.size() / 3;
    if (mode == MODE_POSITION)
      return hostIndexedMeasurement(z_indices, std::move(t), cov_vicon, PB_R_DIAG_BROADCAST, std::move(mask), mem, RBISUpdateInterface::vicon, msg->utime);
    std::vector<double> z((size_t) m * per, 0.0);  // entries at chi indices are ignored (rbis.cpp:203-205)
    if (mode == MODE_POSITION_ORIENT) memcpy(z.data(), t.data(), sizeof(double) * 3 * per);
    return hostIndexedPlusOrientationMeasurement(z_indices, std::move(z), cov_vicon, std::move(q), std::move(mask), mem, RBISUpdateInterface::vicon, msg->utime);
  }
  bool processMessageInit(const msgs::rigid_transform_t *msg, const std::map<std::string, bool> & /*sensors_initialized*/,
                          const RBIS & /*default_state*/, const RBIM & /*default_cov*/, RBIS &init_state, RBIM &init_cov)
  {
    std::vector<double> t, q;
    std::vector<uint8_t> mask;
    int mem;
    if (!to_body(msg, init_state.B, t, q, mask, mem, /*for_init=*/true)) return false;
    init_state.utime = msg->utime;
    const double cov_xyz[3] = { r_xyz2, r_xyz2, r_xyz2 };
    return initPositionOrientation(init_state, init_cov, BatchArray(t.data(), mem), cov_xyz, nullptr, q.data(), r_chi2);
  }
private:
  // msg -> body pose per filter; mask 0 where |translation| < 1e-5 on all axes (":493-494 return NULL")
  bool to_body(const msgs::rigid_transform_t *msg, int B, std::vector<double> &t, std::vector<double> &q, std::vector<uint8_t> &mask,
               int &mem, bool for_init = false) const
  {
    mem = msg->trans.mem;
    if (mem == PB_DEVICE || msg->quat.mem != mem) {
      fprintf(stderr, "ViconHandler: host (or host-broadcast) trans and quat arrays expected\n");
      return false;
    }
    const size_t per = batch_per(mem, B);
    t.resize(3 * per);
    q.resize(4 * per);
    bool any = false;
    if (per > 1) mask.assign(per, 1);
    for (size_t b = 0; b < per; b++) {
      const double tv[3] = { msg->trans.p[b], msg->trans.p[per + b], msg->trans.p[2 * per + b] };
      const double qv[4] = { msg->quat.p[b], msg->quat.p[per + b], msg->quat.p[2 * per + b], msg->quat.p[3 * per + b] };
      double tb[3] = { tv[0], tv[1], tv[2] }, qb[4] = { qv[0], qv[1], qv[2], qv[3] };
      if (apply_frame) {
        bot_quat_rotate_to(qv, body_to_vicon.trans_vec, tb);
        for (int i = 0; i < 3; i++) tb[i] += tv[i];
        quat_mult(qv, body_to_vicon.rot_quat, qb);
      }
      const bool dropped = !for_init && fabs(tv[0]) < 1e-5 && fabs(tv[1]) < 1e-5 && fabs(tv[2]) < 1e-5;
      if (per > 1) mask[b] = !dropped;
      any = any || !dropped;
      for (int i = 0; i < 3; i++) t[(size_t) i * per + b] = tb[i];
      for (int i = 0; i < 4; i++) q[(size_t) i * per + b] = qb[i];
    }
    return any;
  }
};

// PoseMeasHandler (motion_estimate/src/pose_meas/pose_meas.cpp:7-131): a bot_core::pose_t as a position or position +
// orientation measurement, `no_corrections` messages long, then silent.  Same update kernels as the VO / Vicon lists.
class PoseMeasHandler {
public:
  typedef enum { MODE_POSITION, MODE_POSITION_ORIENT } PoseMeasMode;
  PoseMeasMode mode;
  int no_corrections;  // no of corrections to make before going silent
  std::vector<int> z_indices;
  std::vector<double> cov_pose_meas;  // diagonal, of the measured entries
  double r_xyz2, r_chi2;
  explicit PoseMeasHandler(BotParam *param)
  {
    const std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.pose_meas.mode");
    if (mode_str == "position") mode = MODE_POSITION;
    else if (mode_str == "position_orient") mode = MODE_POSITION_ORIENT;
    else {
      mode = MODE_POSITION;
      fprintf(stdout, "Unrecognized PoseMeas mode. Using position mode by default.\n");
    }
    no_corrections = (int) bot_param_get_double_or_fail(param, "state_estimator.pose_meas.no_corrections");
    r_xyz2 = bot_sq(bot_param_get_double_or_fail(param, "state_estimator.pose_meas.r_xyz"));
    r_chi2 = bot_sq(bot_to_radians(bot_param_get_double_or_fail(param, "state_estimator.pose_meas.r_chi")));
    if (mode == MODE_POSITION) { z_indices = RBIS::positionInds(); cov_pose_meas = { r_xyz2, r_xyz2, r_xyz2 }; }
    else { z_indices = { 9, 10, 11, 6, 7, 8 }; cov_pose_meas = { r_xyz2, r_xyz2, r_xyz2, r_chi2, r_chi2, r_chi2 }; }
  }
  RBISUpdateInterface *processMessage(const msgs::pose_t *msg, MavStateEstimator *est)
  {
    // "If we have created no_corrections, go silent afterwards" (:56-64): decrement first, then compare
    no_corrections--;
    if (no_corrections == 1) fprintf(stdout, "Finished making PoseMeas corrections\n");
    if (no_corrections <= 0) return nullptr;
    const int mem = msg->pos.mem;
    if (mem == PB_DEVICE || msg->orientation.mem != mem) {
      fprintf(stderr, "PoseMeasHandler: host (or host-broadcast) pos and orientation arrays expected\n");
      return nullptr;
    }
    const int B = est ? est->B : 1;   // (a host-only caller hands one robot's message over without an estimator)
    const size_t per = batch_per(mem, B);
    // a pose at the origin is "no pose" (:74-75), per filter: mask
    std::vector<uint8_t> mask;
    if (per > 1) mask.assign(per, 1);
    bool any = false;
    for (size_t b = 0; b < per; b++) {
      const bool dropped = fabs(msg->pos.p[b]) < 1e-5 && fabs(msg->pos.p[per + b]) < 1e-5 && fabs(msg->pos.p[2 * per + b]) < 1e-5;
      if (per > 1) mask[b] = !dropped;
      any = any || !dropped;
    }
    if (!any) return nullptr;
    if (mode == MODE_POSITION)
      return hostIndexedMeasurement(z_indices, own_rows(msg->pos, 3, B), cov_pose_meas, PB_R_DIAG_BROADCAST, std::move(mask), mem, RBISUpdateInterface::pose_meas,
                                    msg->utime);
    std::vector<double> z(6 * per, 0.0);  // entries at chi indices are ignored (rbis.cpp:203-205)
    memcpy(z.data(), msg->pos.p, sizeof(double) * 3 * per);
    return hostIndexedPlusOrientationMeasurement(z_indices, std::move(z), cov_pose_meas, own_rows(msg->orientation, 4, B), std::move(mask), mem,
                                                 RBISUpdateInterface::pose_meas, msg->utime);
  }
  // :98-129
  bool processMessageInit(const msgs::pose_t *msg, const std::map<std::string, bool> & /*sensors_initialized*/,
                          const RBIS & /*default_state*/, const RBIM & /*default_cov*/, RBIS &init_state, RBIM &init_cov)
  {
    if (msg->pos.mem == PB_DEVICE || msg->orientation.mem != msg->pos.mem) return false;
    init_state.utime = msg->utime;
    const double cov_xyz[3] = { r_xyz2, r_xyz2, r_xyz2 };
    return initPositionOrientation(init_state, init_cov, msg->pos, cov_xyz, nullptr, msg->orientation.p, r_chi2);
  }
};

class FovisHandler {
public:
  typedef enum { MODE_VELOCITY, MODE_VELOCITY_ROTATION_RATE, MODE_POSITION, MODE_POSITION_ORIENT } FovisMode;
  FovisMode mode;
  std::vector<int> z_indices;
  std::vector<double> cov_fovis;  // diagonal
  int64_t prev_t0_body_utime_ = 0;
  int slot;                       // device snapshot slot holding the filter posterior at prev_timestamp
  // one device block per update, owned by that update and recycled through this pool when the history drops it:
  // z [6][B] (rows 3-5 stay zero) | composed orientation [4][B] | copy of msg->estimate_valid [B]
  std::shared_ptr<DevicePool> pool;

  explicit FovisHandler(BotParam *param, int snapshot_slot = 0) : slot(snapshot_slot)
  {
    std::string mode_str = bot_param_get_str_or_fail(param, "state_estimator.fovis.mode");
    if (mode_str == "velocity_rotation_rate") mode = MODE_VELOCITY_ROTATION_RATE;
    else if (mode_str == "velocity") mode = MODE_VELOCITY;
    else if (mode_str == "position") mode = MODE_POSITION;
    else if (mode_str == "position_orient") mode = MODE_POSITION_ORIENT;
    else {
      fprintf(stdout, "FOVIS mode not understood %s, exiting\n", mode_str.c_str());
      exit(-1);  // rbis_fovis_update.cpp:36-38
    }
    if (mode == MODE_VELOCITY || mode == MODE_VELOCITY_ROTATION_RATE) {
      double r = bot_param_get_double_or_fail(param, "state_estimator.fovis.r_vxyz");
      cov_fovis = { bot_sq(r), bot_sq(r), bot_sq(r) };
      z_indices = RBIS::velocityInds();
      if (mode == MODE_VELOCITY_ROTATION_RATE) {
        double ra = bot_param_get_double_or_fail(param, "state_estimator.fovis.r_vang");
        for (int i = 0; i < 3; i++) cov_fovis.push_back(bot_sq(ra));
        for (int i : RBIS::angularVelocityInds()) z_indices.push_back(i);
      }
    } else {
      double r = bot_param_get_double_or_fail(param, "state_estimator.fovis.r_pxyz");
      cov_fovis = { bot_sq(r), bot_sq(r), bot_sq(r) };
      z_indices = RBIS::positionInds();
      if (mode == MODE_POSITION_ORIENT) {
        double rc = bot_param_get_double_or_fail(param, "state_estimator.fovis.r_chi");  // NOT deg->rad (:99-102)
        for (int i = 0; i < 3; i++) cov_fovis.push_back(bot_sq(rc));
        for (int i : RBIS::chiInds()) z_indices.push_back(i);
      }
    }
  }
  // The estimator calls this when the posterior at a future `prev_timestamp` is the head: the device-side
  // replacement of history.updateMap.lower_bound(prev_timestamp) (rbis_fovis_update.cpp:184-207).
  void markKeyframe(MavStateEstimator *est)
  {
    est->flushPending();
    pb_snapshot(est->ctx, slot);
    prev_t0_body_utime_ = est->head_utime;
  }

  RBISUpdateInterface *processMessage(const msgs::update_t *msg, MavStateEstimator *est)
  {
    const int B = est->B;
    // estimate_status != ESTIMATE_VALID -> NULL (:160-164); per filter that is a mask, and NULL when no filter is valid
    if (msg->estimate_valid != nullptr && std::find_if(msg->estimate_valid, msg->estimate_valid + B,
                                                       [](uint8_t v) { return v != 0; }) == msg->estimate_valid + B) {
      fprintf(stdout, "FovisHandler: FOVIS failure, not integrating this measurement\n");
      return nullptr;
    }
    if (mode == MODE_VELOCITY_ROTATION_RATE) {
      fprintf(stdout, "FovisHandler Mode not supported, exiting\n");  // :276-285
      return nullptr;
    }
    if (mode == MODE_VELOCITY) {
      if (msg->translation.mem == PB_DEVICE) return nullptr;
      const double elapsed = (double) (msg->timestamp - msg->prev_timestamp) * 1E-6;
      const int mem = msg->translation.mem;
      std::vector<double> z = own_rows(msg->translation, 3, B);
      for (double &v : z) v /= elapsed;
      return hostIndexedMeasurement(RBIS::velocityInds(), std::move(z), cov_fovis, PB_R_DIAG_BROADCAST, own_mask(msg->estimate_valid, mem, B), mem,
                                    RBISUpdateInterface::fovis, msg->timestamp);
    }
    // position / position_orient: T1 = T0(posterior at prev_timestamp) * (t, q).  T0 comes from a checkpoint (history) or
    // from the snapshot markKeyframe() took, never from the head: updates the estimator is holding back for fusion
    // (fuse_ins_legodo / fuse_corrections) stay held, so that this measurement can ride in the same kernel.
    if (est->history_slots > 0 && msg->prev_timestamp != prev_t0_body_utime_) {
      // The reference's own look-up (:177-213): the posterior of the first update at or after prev_timestamp, at most
      // 25 ms later, becomes the cached T0 -- here: copied from that update's checkpoint into the snapshot slot.
      auto &map = est->history.updateMap;
      auto lower_it = map.lower_bound(msg->prev_timestamp);
      // an update that applied to NO filter is a message for which the reference's handler returned NULL: it is not in the
      // reference's history, the look-up lands on the update after it
      while (lower_it != map.end() && lower_it->second->appliesToNoFilter(est->ctx, B)) ++lower_it;
      if (lower_it == map.end()) {
        fprintf(stdout, "%lld at the end\n", (long long) msg->prev_timestamp);  // :192-195
        return nullptr;
      }
      const double diff_utime = (double) (lower_it->first - msg->prev_timestamp) * 1E-6;
      if (diff_utime > 0.025) {
        fprintf(stdout, "FOIVS: time difference for VO delta root pose is too great (%fsec). Will not use\n", diff_utime);
        return nullptr;
      }
      // lower_it->second->posterior_state (:196-206): from that update's checkpoint, or re-derived from the nearest earlier
      // one when the checkpoints are sparser than the updates (history_checkpoint_every > 1, the default for a configuration
      // that only sets utime_history_span) or the update is the INS half of a fused pair
      if (!est->snapshotPosteriorOf(lower_it, slot)) {
        fprintf(stdout, "FovisHandler: the posterior of the update at %lld cannot be had (not applied yet, or no free checkpoint "
                        "slot): %s. Will not use\n", (long long) lower_it->first, pb_last_error(est->ctx));
        return nullptr;
      }
      prev_t0_body_utime_ = msg->prev_timestamp;  // :213
    }
    const double diff = (double) (prev_t0_body_utime_ - msg->prev_timestamp) * 1E-6;
    if (diff > 0.025 || diff < -0.025) {  // without a history the keyframe is whatever markKeyframe() last captured
      fprintf(stdout, "FOIVS: time difference for VO delta root pose is too great (%fsec). Will not use\n", diff);  // :186-189
      return nullptr;
    }
    // The measurement (T1's translation and rotation) is formed on the device and belongs to THIS update: a later message
    // must not overwrite it, because the history re-applies the update when an older measurement arrives late.
    if (!pool) pool = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, sizeof(double) * 10 * (size_t) B + (size_t) B);
    bool fresh = false;
    const std::shared_ptr<DeviceBlock> block = take_block(pool, &fresh);
    if (!block) return pb_report("FovisHandler", est->ctx);
    double *d_z6 = (double *) block->p, *d_q = d_z6 + (size_t) 6 * B;
    uint8_t *d_valid = (uint8_t *) (d_q + (size_t) 4 * B);
    if (fresh) {  // rows 3..5 of z are never written again: z at chi indices is ignored (rbis.cpp:203-205)
      std::vector<double> zero((size_t) 6 * B, 0.0);
      pb_memcpy_h2d(est->ctx, d_z6, zero.data(), sizeof(double) * 6 * B);
    }
    if (pb_compose_delta(est->ctx, slot, msg->translation.p, msg->rotation.p, d_z6, d_q, msg->translation.mem) != PB_OK)
      return pb_report("FovisHandler", est->ctx);
    const uint8_t *valid = nullptr;  // the composed z / q live on the device, so does the mask that goes with them
    if (msg->estimate_valid != nullptr && msg->translation.mem != PB_HOST_BROADCAST) {  // broadcast: all valid here
      pb_memcpy_h2d(est->ctx, d_valid, msg->estimate_valid, (size_t) B);
      valid = d_valid;
    }
    RBISIndexedMeasurement *u;
    if (mode == MODE_POSITION)
      u = new RBISIndexedMeasurement(RBIS::positionInds(), BatchArray(d_z6, PB_DEVICE), cov_fovis.data(), PB_R_DIAG_BROADCAST,
                                     valid, RBISUpdateInterface::fovis, msg->timestamp);
    else
      u = new RBISIndexedPlusOrientationMeasurement(z_indices, BatchArray(d_z6, PB_DEVICE), cov_fovis.data(), PB_R_DIAG_BROADCAST,
                                                    BatchArray(d_q, PB_DEVICE), valid, RBISUpdateInterface::fovis,
                                                    msg->timestamp);
    u->owned_dev = block;
    u->owned_R = cov_fovis;  // the update owns its R too (the reference copies cov_fovis into the update object)
    u->measurement_cov = u->owned_R.data();
    return u;
  }
};

// ---------------------------------------------------------------------------------------------------------------
// dispatch: LCMFrontEnd::addSensor / SensorHandler::lcm_message_handler without LCM (lcm_front_end.hpp:82-94,139-203)
// ---------------------------------------------------------------------------------------------------------------
class FrontEnd {
public:
  BotParam *param;
  MavStateEstimator *state_estimator = nullptr;
  explicit FrontEnd(BotParam *p) : param(p) {}
  void setStateEstimator(MavStateEstimator *e) { state_estimator = e; }

  template <class MsgT, class HandlerT>
  std::function<void(const MsgT *)> addSensor(const std::string &sensor_prefix,
                                              RBISUpdateInterface *(HandlerT::*handler_function)(const MsgT *, MavStateEstimator *),
                                              HandlerT *handler)
  {
    const std::string pre = "state_estimator." + sensor_prefix;
    const int downsample_factor = (int) bot_param_get_int_or_fail(param, (pre + ".downsample_factor").c_str());
    const bool roll_forward = bot_param_get_boolean_or_fail(param, (pre + ".roll_forward_on_receive").c_str());
    const int64_t utime_delay = bot_param_get_int_or_fail(param, (pre + ".utime_offset").c_str());
    auto counter = std::make_shared<int64_t>(0);
    return [=](const MsgT *msg) {
      if (state_estimator == nullptr) return;
      if ((*counter)++ % downsample_factor != 0) return;                     // :147
      RBISUpdateInterface *update = (handler->*handler_function)(msg, state_estimator);
      if (update != nullptr) {
        update->utime -= utime_delay;                                        // :157
        state_estimator->addUpdate(update, roll_forward);                    // :158
      }
    };
  }
};

// ---------------------------------------------------------------------------------------------------------------
// wire side (pronto_wire.hpp): publish the head of one filter, replay a recorded LCM log into the batch
// ---------------------------------------------------------------------------------------------------------------

// rbisCreateFilterStateMessageCPP (rbis.cpp:287-304) for filter b: always rbis_num_states = 21 entries and the full
// 21 x 21 column-major covariance; a 15-state batch publishes zero bias entries like the reference run with q_bias = 0.
inline pronto_wire::filter_state_t rbisCreateFilterStateMessageCPP(const RBIS &state, const RBIM &cov, int b)
{
  pronto_wire::filter_state_t msg;
  msg.utime = state.utime;
  msg.num_states = RBIS::rbis_num_states;
  msg.num_cov_elements = msg.num_states * msg.num_states;
  for (int i = 0; i < 4; i++) msg.quat[i] = state.q(i, b);
  msg.state.assign((size_t) msg.num_states, 0.0);
  msg.cov.assign((size_t) msg.num_cov_elements, 0.0);
  for (int i = 0; i < state.n; i++) msg.state[(size_t) i] = state(i, b);
  for (int c = 0; c < cov.n; c++)
    for (int r = 0; r < cov.n; r++) msg.cov[(size_t) c * msg.num_states + r] = cov(r, c, b);
  return msg;
}

// InitMessageHandler (rbis_initializer.cpp:162-184): a pronto::filter_state_t resets the estimator on the fly -- the
// reference's checkpoint / resume mechanism (what FilterStatePublisher writes can be read back here).
// RBIS(msg) (rbis.hpp:69-78): vec <- state[0..n), quat <- msg.quat.  The RigidBodyState(vec) constructor folds a chi beyond
// the tolerance into its own quaternion before msg.quat overwrites that quaternion, i.e. such a chi is dropped; published
// heads carry chi = 0 anyway.
class InitMessageHandler {
public:
  double chi_tol = 1e-6;  // eigen_utils' chiToQuat tolerance: the same constant as pb_set_constants' chi_tol
  // one message for every filter of the batch
  RBISUpdateInterface *processMessage(const pronto_wire::filter_state_t *msg, MavStateEstimator *est)
  {
    return processMessages(std::vector<pronto_wire::filter_state_t>((size_t) est->B, *msg), est);
  }
  // one message per filter (msgs.size() == batch): resume a whole batch from what was published
  RBISUpdateInterface *processMessages(const std::vector<pronto_wire::filter_state_t> &msgs, MavStateEstimator *est)
  {
    const int n = est->n, B = est->B;
    if ((int) msgs.size() != B) return nullptr;
    RBIS x(n, B);
    RBIM P(n, B);
    for (int b = 0; b < B; b++) {
      const pronto_wire::filter_state_t &m = msgs[(size_t) b];
      if (m.num_states != RBIS::rbis_num_states || m.num_cov_elements != m.num_states * m.num_states) {
        fprintf(stderr, "error, constructed RBIS from rbis_filter_state_t of wrong size\n");  // rbis.hpp:72-74
        return nullptr;
      }
      for (int i = 0; i < n; i++) x(i, b) = m.state[(size_t) i];
      const double chi2 = x(6, b) * x(6, b) + x(7, b) * x(7, b) + x(8, b) * x(8, b);
      if (chi2 > chi_tol * chi_tol) x(6, b) = x(7, b) = x(8, b) = 0.0;
      for (int i = 0; i < 4; i++) x.q(i, b) = m.quat[i];
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) P(r, c, b) = m.cov[(size_t) c * m.num_states + r];
    }
    x.utime = msgs[0].utime;
    return new RBISResetUpdate(x, P, RBISUpdateInterface::init_message, msgs[0].utime);
  }
};

// LCMFrontEnd::publishState (lcm_front_end.cpp:144-157), filter-state half: appends the head of the chosen filters
// to an LCM log on `state_estimator.filter_state_channel` when `state_estimator.publish_filter_state` is set.
class FilterStatePublisher {
public:
  std::string filter_state_channel;
  bool publish_filter_state;
  FilterStatePublisher(BotParam *param, pronto_wire::LogWriter *log, std::vector<int> filters)
      : filter_state_channel(bot_param_get_str_or_fail(param, "state_estimator.filter_state_channel")),
        publish_filter_state(bot_param_get_boolean_or_fail(param, "state_estimator.publish_filter_state")),
        log_(log), filters_(std::move(filters)) {}
  // one channel per filter beyond the first so that a reader can tell them apart: CHANNEL, CHANNEL_1, CHANNEL_2 ...
  void publishHead(MavStateEstimator *est)
  {
    if (!publish_filter_state || log_ == nullptr) return;
    RBIS s;
    RBIM c;
    est->getHeadState(s, c);
    std::vector<uint8_t> buf;
    for (size_t k = 0; k < filters_.size(); k++) {
      rbisCreateFilterStateMessageCPP(s, c, filters_[k]).encode(buf);
      log_->write(s.utime, k == 0 ? filter_state_channel : filter_state_channel + "_" + std::to_string(k), buf);
    }
  }
private:
  pronto_wire::LogWriter *log_;
  std::vector<int> filters_;
};

// motion_estimate/scripts/drift_per_distance.py for every filter of the batch: the reference's accuracy evaluation (POSE_BODY against
// POSE_GROUND_TRUTH, published as pronto::error_metrics_t on PRONTO_ERROR) as a handler on the ground-truth pose channel.  It is not
// a sensor: processMessage creates no update and nothing enters the history; it scores the device head on the device
// (pb_score_ground_truth) and leaves the filter as it is.  Wire it as a subscribePose callback of LogPlayer, SegmentBatcher or
// SegmentStreamer; a filter whose segment has no message (valid = 0) is not touched.  A message it cannot take (pos and
// orientation in different memory spaces, a PB_DEVICE pose that is not one [7][B] block, a failed call) is dropped with
// est->last_status set; `valid` is honoured for host messages only, as msgs::pose_t documents it.
//   thresholds: the script's (parameterTimeElapsedThreshold = 10.0; the distance test off) unless the optional keys
//   state_estimator.error_metrics.time_elapsed_threshold / .distance_threshold are present
class DriftPerDistance {
public:
  double time_elapsed_threshold = 10.0, distance_threshold = 0.0;
  bool absolute = true;              // also keep the absolute error (PB_SCORE_ABS; an addition to the script)
  std::string error_channel = "PRONTO_ERROR";
  int64_t messages = 0, published = 0;
  explicit DriftPerDistance(BotParam *param)
  {
    time_elapsed_threshold = bot_param_get_double_or(param, "state_estimator.error_metrics.time_elapsed_threshold", time_elapsed_threshold);
    distance_threshold = bot_param_get_double_or(param, "state_estimator.error_metrics.distance_threshold", distance_threshold);
  }
  // PRONTO_ERROR events of ONE chosen filter go to `log` whenever that filter closes a window (one small read-back per ground-truth
  // message; without it processMessage never synchronises)
  void publish(pronto_wire::LogWriter *log, int filter)
  {
    log_ = log;
    publish_filter_ = filter;
  }
  // on_pose_gt (drift_per_distance.py:70-138).  The device head is brought up to date first, exactly as getHeadState does: the shim
  // may be holding an INS step back to fuse it with the leg odometry, and the score must see what POSE_BODY would have carried.
  void processMessage(const msgs::pose_t *ground_truth, MavStateEstimator *est)
  {
    const int B = est->B;
    if (!ready_) {
      const int rc0 = pb_score_init(est->ctx, time_elapsed_threshold, distance_threshold);
      if (rc0 != PB_OK) {  // (a negative threshold key, or no memory: the message is refused, the estimator goes on)
        pb_report("DriftPerDistance", est->ctx);
        est->last_status = rc0;
        return;
      }
      ready_ = true;
    }
    est->flushPending();
    const int mem = ground_truth->pos.mem;
    if (ground_truth->orientation.mem != mem) {
      fprintf(stderr, "DriftPerDistance: pos and orientation must live in the same memory space\n");
      est->last_status = PB_ERR_ARG;
      return;
    }
    const double *pose7 = nullptr;
    if (mem == PB_HOST_BROADCAST) {
      for (int i = 0; i < 3; i++) one_[i] = ground_truth->pos.p[i];
      for (int i = 0; i < 4; i++) one_[3 + i] = ground_truth->orientation.p[i];
      pose7 = one_;
    } else if (ground_truth->orientation.p == ground_truth->pos.p + (size_t) 3 * B) {
      pose7 = ground_truth->pos.p;  // already one [7][B] block
    } else if (mem == PB_HOST) {
      block_.resize((size_t) 7 * B);
      memcpy(block_.data(), ground_truth->pos.p, sizeof(double) * 3 * (size_t) B);
      memcpy(block_.data() + (size_t) 3 * B, ground_truth->orientation.p, sizeof(double) * 4 * (size_t) B);
      pose7 = block_.data();
    } else {
      fprintf(stderr, "DriftPerDistance: a PB_DEVICE pose must be one [7][B] block (pos, then orientation)\n");
      est->last_status = PB_ERR_ARG;
      return;
    }
    const int flags = PB_SCORE_DRIFT | (absolute ? PB_SCORE_ABS : 0);
    // msgs::pose_t::valid is a HOST array and belongs to PB_HOST messages; a PB_DEVICE message is scored for every filter
    const uint8_t *valid = mem == PB_DEVICE ? nullptr : ground_truth->valid;
    int rc = pb_score_ground_truth(est->ctx, ground_truth->utime, nullptr, pose7, valid, PB_SLOT_HEAD, flags, mem);
    if (rc != PB_OK) {
      est->last_status = rc;
      return;
    }
    messages++;
    if (log_ != nullptr && publish_filter_ >= 0 && publish_filter_ < B) {
      pronto_wire::error_metrics_t em;
      if (newest(est, publish_filter_, em) && em.utime != last_published_) {
        std::vector<uint8_t> buf;
        em.encode(buf);
        log_->write(em.utime, error_channel, buf);
        last_published_ = em.utime;
        published++;
      }
    }
  }
  // the newest error_metrics_t of one filter; false: no window has closed yet (or an error, est->last_status)
  bool newest(MavStateEstimator *est, int filter, pronto_wire::error_metrics_t &em) const
  {
    double o[10];
    int64_t utime = -2;
    const int rc = pb_score_last(est->ctx, filter, &utime, o);
    if (rc != PB_OK) {
      est->last_status = rc;
      return false;
    }
    if (utime < 0) return false;
    em.utime = utime;
    for (int i = 0; i < 3; i++) { em.pos_error[i] = o[i]; em.rpy_error[i] = o[4 + i]; }
    em.pos_error_norm = o[3];
    em.distance_travelled = o[7];
    em.percent_ddt = o[8];
    em.time_elapsed = o[9];
    return true;
  }
  pronto_wire::error_metrics_t metrics(MavStateEstimator *est, int filter) const
  {
    pronto_wire::error_metrics_t em;
    em.utime = -2;
    newest(est, filter, em);
    return em;
  }
  // the accumulators of filters [first, first + count): rows [PB_SCORE_ROWS][count], counts [PB_SCORE_COUNTS][count] (enum pb_score_row / _count)
  bool rows(MavStateEstimator *est, int first, int count, std::vector<double> &rows_out, std::vector<int64_t> &counts_out) const
  {
    rows_out.assign((size_t) PB_SCORE_ROWS * count, 0.0);
    counts_out.assign((size_t) PB_SCORE_COUNTS * count, 0);
    const int rc = pb_score_get(est->ctx, first, count, rows_out.data(), counts_out.data(), PB_HOST);
    if (rc != PB_OK) est->last_status = rc;
    return rc == PB_OK;
  }
  // the filter with the smallest metric (enum pb_score_metric) and its value; -1: no filter has data
  int best(MavStateEstimator *est, int metric, double *value = nullptr) const
  {
    int f = -1;
    const int rc = pb_score_best(est->ctx, metric, &f, value);
    if (rc != PB_OK) est->last_status = rc;
    return rc == PB_OK ? f : -1;
  }

private:
  bool ready_ = false;
  double one_[7] = { 0, 0, 0, 1, 0, 0, 0 };
  std::vector<double> block_;
  pronto_wire::LogWriter *log_ = nullptr;
  int publish_filter_ = -1;
  int64_t last_published_ = -2;
};

// Log replay (lcm_front_end.cpp:223-229 handle loop, reading a recorded segment instead of the network): events are
// dispatched in file order to the subscribed channels.  One recorded robot feeds EVERY filter of the batch -- the
// batch differs in parameters / initial state, not in data (param_sweep.py:39-52) -- so a decoded message is handed to
// the callback LCMFrontEnd::addSensor returns as PB_HOST_BROADCAST blocks ([rows] values, expanded on the device:
// nothing of batch size is built on the host or crosses PCIe).
class LogPlayer {
public:
  explicit LogPlayer(int batch) : B_(batch) {}
  void subscribeRaw(const std::string &channel, std::function<void(const pronto_wire::LogEvent &)> cb)
  {
    subs_[channel] = std::move(cb);
  }
  void subscribeIndexedMeasurement(const std::string &channel, std::function<void(const msgs::indexed_measurement_t *)> cb)
  {
    subs_[channel] = [this, cb](const pronto_wire::LogEvent &ev) {
      pronto_wire::indexed_measurement_t w;
      if (w.decode(ev.data.data(), ev.data.size()) < 0 || w.measured_cov_dim != w.measured_dim * w.measured_dim) {
        n_bad_++;
        return;
      }
      // one recorded message for every filter: hand the [m] / [m*m] values over as PB_HOST_BROADCAST blocks
      msgs::indexed_measurement_t msg;
      msg.utime = w.utime;
      msg.z_indices.assign(w.z_indices.begin(), w.z_indices.end());
      msg.z_effective = BatchArray(w.z_effective.data(), PB_HOST_BROADCAST);
      msg.R_effective = w.R_effective.data();
      cb(&msg);
    };
  }
  // Messages whose .lcm definition the caller supplies at run time (lcm_schema.hpp; libbot's bot_core types are not in
  // the reference tree): decoded into a value tree and handed over with the raw event.  `schema` must outlive the player.
  void subscribeSchema(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                       std::function<void(const pronto_wire::Value &, const pronto_wire::LogEvent &)> cb)
  {
    subs_[channel] = [this, schema, type, cb](const pronto_wire::LogEvent &ev) {
      pronto_wire::Value v;
      if (!schema->decode(type, ev.data.data(), ev.data.size(), v)) {
        n_bad_++;
        return;
      }
      cb(v, ev);
    };
  }
  // bot_core::ins_t by field name (utime, gyro[3], accel[3]: what InsHandler::processMessage reads, sensor_handlers.cpp:96-131)
  void subscribeIns(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                    std::function<void(const msgs::ins_t *)> cb)
  {
    subscribeSchema(channel, schema, type, [this, cb](const pronto_wire::Value &v, const pronto_wire::LogEvent &) {
      double g[3], a[3];
      int64_t utime;
      if (!v.integer("utime", utime) || !v.numbers("gyro", g, 3) || !v.numbers("accel", a, 3)) {
        n_bad_++;
        return;
      }
      msgs::ins_t m{ utime, BatchArray(g, PB_HOST_BROADCAST), BatchArray(a, PB_HOST_BROADCAST) };
      cb(&m);
    });
  }
  // bot_core::pose_t (utime, pos[3], vel[3], orientation[4]: ScanMatcherHandler::processMessage, sensor_handlers.cpp:689-724)
  void subscribePose(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                     std::function<void(const msgs::pose_t *)> cb)
  {
    subscribeSchema(channel, schema, type, [this, cb](const pronto_wire::Value &v, const pronto_wire::LogEvent &) {
      double p[3], vel[3], q[4];
      int64_t utime;
      if (!v.integer("utime", utime) || !v.numbers("pos", p, 3) || !v.numbers("vel", vel, 3) || !v.numbers("orientation", q, 4)) {
        n_bad_++;
        return;
      }
      msgs::pose_t m{ utime, BatchArray(p, PB_HOST_BROADCAST), BatchArray(vel, PB_HOST_BROADCAST), BatchArray(q, PB_HOST_BROADCAST) };
      cb(&m);
    });
  }
  // bot_core::rigid_transform_t (utime, trans[3], quat[4]: ViconHandler::processMessage, sensor_handlers.cpp:476-536)
  void subscribeRigidTransform(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                               std::function<void(const msgs::rigid_transform_t *)> cb)
  {
    subscribeSchema(channel, schema, type, [this, cb](const pronto_wire::Value &v, const pronto_wire::LogEvent &) {
      double t[3], q[4];
      int64_t utime;
      if (!v.integer("utime", utime) || !v.numbers("trans", t, 3) || !v.numbers("quat", q, 4)) {
        n_bad_++;
        return;
      }
      msgs::rigid_transform_t m{ utime, BatchArray(t, PB_HOST_BROADCAST), BatchArray(q, PB_HOST_BROADCAST) };
      cb(&m);
    });
  }
  // bot_core::kvh_raw_imu_batch_t (utime, raw_imu[]{utime, packet_count, delta_rotation[3], linear_acceleration[3]}:
  // IMUStream::convertFromLCMBatch, imu_stream.cpp:62-98; newest packet first, as on the wire)
  void subscribeKvhBatch(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                         std::function<void(const msgs::kvh_raw_imu_batch_t *)> cb)
  {
    subscribeSchema(channel, schema, type, [this, cb](const pronto_wire::Value &v, const pronto_wire::LogEvent &) {
      msgs::kvh_raw_imu_batch_t m;
      m.mem = PB_HOST_BROADCAST;
      const pronto_wire::Value *raw = v.get("raw_imu");
      if (!v.integer("utime", m.utime) || raw == nullptr || raw->kind != pronto_wire::Value::ARRAY) {
        n_bad_++;
        return;
      }
      std::vector<double> store(raw->items.size() * 6);
      for (size_t k = 0; k < raw->items.size(); k++) {
        const pronto_wire::Value &pk = raw->items[k];
        msgs::kvh_raw_imu_packet_t p;
        if (!pk.integer("utime", p.utime) || !pk.integer("packet_count", p.packet_count) ||
            !pk.numbers("delta_rotation", &store[k * 6], 3) || !pk.numbers("linear_acceleration", &store[k * 6 + 3], 3)) {
          n_bad_++;
          return;
        }
        p.delta_rotation = &store[k * 6];
        p.linear_acceleration = &store[k * 6 + 3];
        m.raw_imu.push_back(p);
      }
      cb(&m);
    });
  }
  void subscribeUpdate(const std::string &channel, std::function<void(const msgs::update_t *)> cb)
  {
    subs_[channel] = [this, cb](const pronto_wire::LogEvent &ev) {
      pronto_wire::update_t w;
      if (w.decode(ev.data.data(), ev.data.size()) < 0) {
        n_bad_++;
        return;
      }
      // estimate_status != ESTIMATE_VALID for the one robot = for every filter: an all-zero per-filter mask
      if (w.estimate_status != pronto_wire::update_t::ESTIMATE_VALID) valid_.assign((size_t) B_, (uint8_t) 0);
      msgs::update_t msg;
      msg.timestamp = w.timestamp;
      msg.prev_timestamp = w.prev_timestamp;
      msg.estimate_valid = (w.estimate_status == pronto_wire::update_t::ESTIMATE_VALID) ? nullptr : valid_.data();
      msg.translation = BatchArray(w.translation, PB_HOST_BROADCAST);
      msg.rotation = BatchArray(w.rotation, PB_HOST_BROADCAST);
      cb(&msg);
    };
  }
  // the two status channels of YawLockHandler (fixed-size pronto types, pronto_wire.hpp)
  void subscribeControllerStatus(const std::string &channel, std::function<void(const msgs::controller_status_t *)> cb)
  {
    subs_[channel] = [this, cb](const pronto_wire::LogEvent &ev) {
      pronto_wire::controller_status_t w;
      if (w.decode(ev.data.data(), ev.data.size()) < 0) {
        n_bad_++;
        return;
      }
      msgs::controller_status_t m;
      m.utime = w.utime; m.state = w.state; m.controller_utime = w.controller_utime; m.V = w.V; m.Vdot = w.Vdot;
      cb(&m);
    };
  }
  void subscribeBehavior(const std::string &channel, std::function<void(const msgs::behavior_t *)> cb)
  {
    subs_[channel] = [this, cb](const pronto_wire::LogEvent &ev) {
      pronto_wire::behavior_t w;
      if (w.decode(ev.data.data(), ev.data.size()) < 0) {
        n_bad_++;
        return;
      }
      msgs::behavior_t m;
      m.utime = w.utime; m.behavior = w.behavior;
      cb(&m);
    };
  }
  // returns the number of events dispatched, or -1 if the file cannot be opened
  int64_t run(const std::string &path)
  {
    pronto_wire::LogReader rd(path);
    if (!rd.good()) return -1;
    pronto_wire::LogEvent ev;
    int64_t n = 0;
    while (rd.next(ev)) {
      auto it = subs_.find(ev.channel);
      if (it == subs_.end()) continue;
      it->second(ev);
      n++;
    }
    return n;
  }
  int64_t undecodable() const { return n_bad_; }
private:
  int B_;
  int64_t n_bad_ = 0;
  std::map<std::string, std::function<void(const pronto_wire::LogEvent &)>> subs_;
  std::vector<uint8_t> valid_;
};

}  // namespace MavStateEst
