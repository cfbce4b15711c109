// segment_channels.hpp -- what SegmentBatcher (segment_batcher.hpp) and SegmentStreamer (segment_stream.hpp) share: ONE decoder per
// wire type, what a log segment remembers about a channel between messages, and the keeper of the finished runs' results.
//
// A decoder turns (payload bytes, length, the segment's channel state) into the message utime and a fixed byte RECORD: the members the
// handlers read, 8-byte members first (natural alignment), at the named offsets of its layout.  A batched message is its columns'
// records transposed into a [rows][B] block, filter index fastest: the element at record offset o of filter s sits at
// block + o * B + s * sizeof(element).  The streamer's chunk blocks and the batcher's page-locked blocks have this one layout, so both
// build their messages from a block with the same offsets.  Decoding goes through the run-time .lcm schema (lcm_schema.hpp): the
// layout of the stream's last message is verified or rebuilt, the wanted numbers are then read in place (floats stay floats, utimes
// are read as integers); a member with fewer numbers than the record has room for rejects the message.  Where the two replayers differ
// -- a column without a message, a foreign joint list, more new KVH packets than rows -- the decoders report and the callers decide.
#pragma once

#include "mav_state_est_batch.hpp"

namespace MavStateEst {
namespace segment_channels {

using pronto_wire::Schema;
typedef Schema::Plan Plan;

struct Plane { int elem, count; };   // `count` elements of `elem` bytes, back to back: a record's layout is a list of these

inline uint64_t names_hash(const std::vector<std::string> &names)
{
  uint64_t h = 1469598103934665603ull;   // FNV-1a over the names and their boundaries
  for (const std::string &nm : names) {
    for (unsigned char ch : nm) h = (h ^ ch) * 1099511628211ull;
    h = (h ^ 0xffu) * 1099511628211ull;
  }
  return h;
}

// What one segment remembers about one channel between messages: the byte layout of its last message (a recorded stream repeats it), the
// hash of the joint list that came with it, its own IMUStream state (imu_stream.hpp:10-37).  Every message touches it: kept small.
struct ChannelState {
  Plan::Shape shape;
  uint64_t names_hash = 0;
  IMUStreamRule imu;
  int64_t overflow = 0;   // KVH messages with more new packets than the record has rows (the surplus newest ones were left out)
};

// a decoder's compiled member list, and the layout step of its decode: NULL = not a message of the type; else the stream's layout in
// st.shape is this message's -- verified, or rebuilt the long way (*rebuilt: the returned members then hold the decoded strings)
struct PlanChannel {
  Plan plan;
  PlanChannel(const Schema *schema, const std::string &type, const std::vector<std::string> &members, const char *who, const char *what)
      : plan(schema->compile(type, members))
  {
    if (!plan.ok()) fprintf(stderr, "%s: %s %s\n", who, type.c_str(), what);
  }
  const std::vector<Schema::Extracted> *layout(const uint8_t *data, size_t len, ChannelState &st, bool *rebuilt = nullptr) const
  {
    static thread_local std::vector<Schema::Extracted> x;
    return plan.layout(data, len, st.shape, x, rebuilt) ? &x : nullptr;
  }
};
template <class T>
inline T *member(uint8_t *base, size_t off, size_t B = 1) { return (T *) (base + off * B); }
template <class T>
inline const T *member(const uint8_t *base, size_t off, size_t B = 1) { return (const T *) (base + off * B); }

// bot_core::ins_t (utime, gyro[3], accel[3]).  record: f64 gyro[3] accel[3] | u8 valid
struct InsChannel : PlanChannel {
  enum : size_t { GYRO = 0, ACCEL = 24, VALID = 48, BYTES = 49 };
  static std::vector<Plane> planes() { return { { 8, 6 }, { 1, 1 } }; }
  InsChannel(const Schema *schema, const std::string &type, const char *who)
      : PlanChannel(schema, type, { "utime", "gyro", "accel" }, who, "has no utime / gyro / accel members") {}
  bool decode(const uint8_t *data, size_t len, ChannelState &st, uint8_t *rec, int64_t &utime) const
  {
    if (!layout(data, len, st)) return false;
    double v[6];
    if (Plan::gather_i64(st.shape, data, 0, &utime, 1) != 1 || Plan::gather_f64(st.shape, data, 1, v, 3) != 3 || Plan::gather_f64(st.shape, data, 2, v + 3, 3) != 3)
      return false;
    memcpy(rec + GYRO, v, sizeof v);
    rec[VALID] = 1;
    return true;
  }
  static void blank(uint8_t *rec) { rec[VALID] = 0; }   // (a filter without a message idles on its own last sample)
  static msgs::ins_t message(int64_t utime, const uint8_t *block, size_t B, int mem)
  {
    msgs::ins_t m{ utime, BatchArray(member<double>(block, GYRO, B), mem), BatchArray(member<double>(block, ACCEL, B), mem) };
    m.valid = member<uint8_t>(block, VALID, B);
    return m;
  }
};

// bot_core::kvh_raw_imu_batch_t (utime, raw_imu[]{utime, packet_count, delta_rotation[3], linear_acceleration[3]}; raw_imu[0] is the
// NEWEST packet), reduced to what InsHandler::processMessageAtlasSegments reads.  atlas_filter = the handler's: true = the segment's
// own IMUStream de-duplication (imu_stream.cpp:62-98), the new packets' accelerations oldest first for the notch cascade; false =
// newest packet, raw_dt from the two newest (sensor_handlers.cpp:199-204).  max_packets: rows of the new-packet block.
// record: f64 new_accel[max_packets][3] | f64 delta_rotation[3] | f64 raw_dt | i64 utime | i32 n_new | u8 valid
// new_accel rows behind n_new, and delta_rotation / raw_dt of a message without a new packet, are left as they are.
struct KvhChannel : PlanChannel {
  const int max_packets;
  const bool atlas_filter;
  const size_t ACCEL = 0, DELTA_ROTATION, RAW_DT, UTIME, N_NEW, VALID, BYTES;
  std::vector<Plane> planes() const { return { { 8, 3 * max_packets + 5 }, { 4, 1 }, { 1, 1 } }; }
  KvhChannel(const Schema *schema, const std::string &type, bool atlas_filter_, int max_packets_, const char *who)
      : PlanChannel(schema, type, { "utime", "raw_imu.utime", "raw_imu.packet_count", "raw_imu.delta_rotation", "raw_imu.linear_acceleration" }, who,
                    "is not a kvh_raw_imu_batch_t"),
        max_packets(max_packets_ < 1 ? 1 : max_packets_), atlas_filter(atlas_filter_), DELTA_ROTATION((size_t) 24 * max_packets), RAW_DT(DELTA_ROTATION + 24),
        UTIME(RAW_DT + 8), N_NEW(UTIME + 8), VALID(N_NEW + 4), BYTES(VALID + 1) {}
  bool decode(const uint8_t *data, size_t len, ChannelState &st, uint8_t *rec, int64_t &utime) const
  {
    static thread_local std::vector<int64_t> put, pcnt;
    static thread_local std::vector<double> dr, la;
    if (!layout(data, len, st) || Plan::gather_i64(st.shape, data, 0, &utime, 1) != 1) return false;
    size_t np = 0;
    for (const auto &o : st.shape.ops)
      if (o.slot == 1) np += o.count;
    if (np < 1) return false;
    put.resize(np); pcnt.resize(np); dr.resize(3 * np); la.resize(3 * np);
    if (Plan::gather_i64(st.shape, data, 1, put.data(), np) != np || Plan::gather_i64(st.shape, data, 2, pcnt.data(), np) != np ||
        Plan::gather_f64(st.shape, data, 3, dr.data(), 3 * np) != 3 * np || Plan::gather_f64(st.shape, data, 4, la.data(), 3 * np) != 3 * np)
      return false;
    double *acc = member<double>(rec, ACCEL), *drot = member<double>(rec, DELTA_ROTATION), *raw_dt = member<double>(rec, RAW_DT);
    int32_t n_new = 0;
    if (!atlas_filter) {
      if (np < 2) return false;
      for (int i = 0; i < 3; i++) { acc[i] = la[(size_t) i]; drot[i] = dr[(size_t) i]; }
      *raw_dt = (double) (put[0] - put[1]) * 1E-6;
      n_new = 1;
    } else {
      st.imu.resetIfBackwards(pcnt[0]);
      for (size_t i = np; i-- > 0;) {   // oldest first
        int64_t utime_delta;
        if (!st.imu.accept(pcnt[i], put[i], utime_delta)) continue;
        if (n_new < max_packets)
          for (int a = 0; a < 3; a++) acc[(size_t) 3 * n_new + a] = la[3 * i + a];
        n_new++;
        for (int a = 0; a < 3; a++) drot[a] = dr[3 * i + a];   // (of the newest new packet in the end)
        *raw_dt = (double) utime_delta * 1E-6;
      }
      if (n_new > max_packets) { st.overflow++; n_new = max_packets; }
    }
    memcpy(rec + UTIME, &utime, 8);
    memcpy(rec + N_NEW, &n_new, 4);
    rec[VALID] = n_new > 0;
    return true;
  }
  void blank(uint8_t *rec) const { const int32_t z = 0; memcpy(rec + N_NEW, &z, 4); rec[VALID] = 0; }
  msgs::kvh_raw_imu_segments_t message(int64_t utime, const uint8_t *block, size_t B, int mem) const
  {
    return { utime, max_packets, member<int32_t>(block, N_NEW, B), member<uint8_t>(block, VALID, B), member<double>(block, ACCEL, B),
             member<double>(block, DELTA_ROTATION, B), member<double>(block, RAW_DT, B), member<int64_t>(block, UTIME, B), mem };
  }
};

// bot_core::joint_state_t (utime, joint_name[], joint_position[], joint_velocity[], joint_effort[]).
// record of a list of n joints: i64 utime | f32 position[n] velocity[n] effort[n] | u8 valid
// In two steps, because the replayers differ in whose joint list a message is held to: open() makes st.names_hash the hash of THIS
// message's list (decoded only when the stream's layout changed, normally once per segment: *fresh is then the list, else NULL),
// read() fills the record.
struct JointStateChannel : PlanChannel {
  struct Layout {
    size_t n, UTIME = 0, POSITION = 8, VELOCITY, EFFORT, VALID, BYTES;
    explicit Layout(size_t joints) : n(joints), VELOCITY(8 + 4 * n), EFFORT(8 + 8 * n), VALID(8 + 12 * n), BYTES(9 + 12 * n) {}
    std::vector<Plane> planes() const { return { { 8, 1 }, { 4, (int) (3 * n) }, { 1, 1 } }; }
  };
  JointStateChannel(const Schema *schema, const std::string &type, const char *who)
      : PlanChannel(schema, type, { "utime", "joint_name", "joint_position", "joint_velocity", "joint_effort" }, who, "is not a joint_state_t") {}
  bool open(const uint8_t *data, size_t len, ChannelState &st, const std::vector<std::string> **fresh = nullptr) const
  {
    bool rebuilt = false;
    const std::vector<Schema::Extracted> *x = layout(data, len, st, &rebuilt);
    if (!x) return false;
    if (rebuilt) st.names_hash = names_hash((*x)[1].str);
    if (fresh) *fresh = rebuilt ? &(*x)[1].str : nullptr;
    return true;
  }
  bool read(const uint8_t *data, const ChannelState &st, const Layout &lay, uint8_t *rec, int64_t &utime) const
  {
    const size_t n = lay.n;
    float *f = member<float>(rec, lay.POSITION);
    if (Plan::gather_i64(st.shape, data, 0, &utime, 1) != 1 || Plan::gather_f32(st.shape, data, 2, f, n) != n ||
        Plan::gather_f32(st.shape, data, 3, f + n, n) != n || Plan::gather_f32(st.shape, data, 4, f + 2 * n, n) != n)
      return false;
    memcpy(rec + lay.UTIME, &utime, 8);
    rec[lay.VALID] = 1;
    return true;
  }
  static void blank(const Layout &lay, uint8_t *rec) { rec[lay.VALID] = 0; }   // (the block keeps this filter's last message; it is masked)
  // the message over [3 n][B] floats `values` in `mem` and a block `times` in `times_mem` that holds the records' utime and valid members
  static msgs::joint_state_t message(int64_t utime, const std::vector<std::string> &names, const Layout &lay, size_t B, const float *values, int mem,
                                     const uint8_t *times, int times_mem)
  {
    return { utime, names, values, values + lay.n * B, values + 2 * lay.n * B, mem, member<int64_t>(times, lay.UTIME, B), member<uint8_t>(times, lay.VALID, B), times_mem };
  }
};

// bot_core::six_axis_force_torque_array_t: force z of sensors 0 / 1 = left / right foot, as on the wire (signed doubles).  No record
// of its own: the batcher hands the doubles on, the streamer keeps what the handler keeps of them, (float) fabs().
struct ForceTorqueChannel : PlanChannel {
  ForceTorqueChannel(const Schema *schema, const std::string &type, const char *who)
      : PlanChannel(schema, type, { "utime", "sensors.force" }, who, "is not a six_axis_force_torque_array_t") {}
  bool decode(const uint8_t *data, size_t len, ChannelState &st, double force_z[2], int64_t &utime) const
  {
    if (!layout(data, len, st)) return false;
    double f[6];
    if (Plan::gather_i64(st.shape, data, 0, &utime, 1) != 1 || Plan::gather_f64(st.shape, data, 1, f, 6) != 6) return false;
    force_z[0] = f[2];   // sensors[0].force[2]
    force_z[1] = f[5];   // sensors[1].force[2]
    return true;
  }
};

// bot_core::pose_t (utime, pos[3], vel[3], orientation[4]).  record: f64 pos[3] vel[3] orientation[4] | u8 valid
struct PoseChannel : PlanChannel {
  enum : size_t { POS = 0, VEL = 24, ORIENTATION = 48, VALID = 80, BYTES = 81 };
  static std::vector<Plane> planes() { return { { 8, 10 }, { 1, 1 } }; }
  PoseChannel(const Schema *schema, const std::string &type, const char *who)
      : PlanChannel(schema, type, { "utime", "pos", "vel", "orientation" }, who, "is not a pose_t") {}
  bool decode(const uint8_t *data, size_t len, ChannelState &st, uint8_t *rec, int64_t &utime) const
  {
    if (!layout(data, len, st)) return false;
    double v[10];
    if (Plan::gather_i64(st.shape, data, 0, &utime, 1) != 1 || Plan::gather_f64(st.shape, data, 1, v, 3) != 3 || Plan::gather_f64(st.shape, data, 2, v + 3, 3) != 3 ||
        Plan::gather_f64(st.shape, data, 3, v + 6, 4) != 4)
      return false;
    memcpy(rec + POS, v, sizeof v);
    rec[VALID] = 1;
    return true;
  }
  static void blank(uint8_t *rec) { memset(rec, 0, BYTES); *member<double>(rec, ORIENTATION) = 1.0; }   // no message: zero pose, identity quaternion
  static msgs::pose_t message(int64_t utime, const uint8_t *block, size_t B)   // (host blocks only: the handler copies what it keeps)
  {
    msgs::pose_t m{ utime, BatchArray(member<double>(block, POS, B), PB_HOST), BatchArray(member<double>(block, VEL, B), PB_HOST),
                    BatchArray(member<double>(block, ORIENTATION, B), PB_HOST) };
    m.valid = member<uint8_t>(block, VALID, B);
    return m;
  }
};

// pronto::update_t (pronto_wire.hpp).  record: f64 translation[3] rotation[4] | u8 valid (estimate_status == ESTIMATE_VALID)
// A batched message's timestamp / prev_timestamp are the LEAD's on the batch's time base: *prev_behind = prev_timestamp - timestamp.
struct UpdateChannel {
  enum : size_t { TRANSLATION = 0, ROTATION = 24, VALID = 56, BYTES = 57 };
  static std::vector<Plane> planes() { return { { 8, 7 }, { 1, 1 } }; }
  static bool decode(const uint8_t *data, size_t len, uint8_t *rec, int64_t &utime, int64_t *prev_behind)
  {
    pronto_wire::update_t w;
    if (w.decode(data, len) < 0) return false;
    utime = w.timestamp;
    if (prev_behind) *prev_behind = w.prev_timestamp - w.timestamp;
    memcpy(rec + TRANSLATION, w.translation, 24);
    memcpy(rec + ROTATION, w.rotation, 32);
    rec[VALID] = w.estimate_status == pronto_wire::update_t::ESTIMATE_VALID;
    return true;
  }
  static void blank(uint8_t *rec) { memset(rec, 0, BYTES); *member<double>(rec, ROTATION) = 1.0; }
  static msgs::update_t message(int64_t utime, int64_t prev_behind, const uint8_t *block, size_t B)
  {
    return msgs::update_t{ utime, utime + prev_behind, member<uint8_t>(block, VALID, B), BatchArray(member<double>(block, TRANSLATION, B), PB_HOST),
                           BatchArray(member<double>(block, ROTATION, B), PB_HOST) };
  }
};

// The RESULT of a run is its filter's head at the end of ITS log: finalize() the moment a segment has no event left.
class Results {
public:
  Results(int n, int B) : state_(n, B), cov_(n, B), ll_((size_t) B, 0.0), utime_((size_t) B, 0), finished_((size_t) B, 0)
  {
    state_.quat.assign(state_.quat.size(), 0.0);   // (columns of segments never added are zero)
  }
  bool finished(int s) const { return finished_[(size_t) s] != 0; }
  // the runs of segments [first, first + count) are complete: read their heads (applies whatever the estimator holds back first)
  void finalize(MavStateEstimator *est, int first, int count, const char *who)
  {
    const int n = est->n, B = est->B;
    est->flushPending();
    std::vector<double> v((size_t) n * count), q((size_t) 4 * count), c((size_t) n * n * count), l((size_t) count);
    if (pb_get_head(est->ctx, first, count, v.data(), q.data(), c.data(), l.data(), PB_HOST) != PB_OK) {
      fprintf(stderr, "%s: %s\n", who, pb_last_error(est->ctx));
      return;
    }
    for (int k = 0; k < count; k++) {
      const size_t s = (size_t) (first + k);
      for (int i = 0; i < n; i++) state_.vec[(size_t) i * B + s] = v[(size_t) i * count + k];
      for (int i = 0; i < 4; i++) state_.quat[(size_t) i * B + s] = q[(size_t) i * count + k];
      for (int i = 0; i < n * n; i++) cov_.m[(size_t) i * B + s] = c[(size_t) i * count + k];
      ll_[s] = l[(size_t) k];
      utime_[s] = est->head_utime;
      finished_[s] = 1;
    }
  }
  // the head of every segment's filter at the end of ITS log (valid after run(); columns of segments never added are zero)
  void finalState(RBIS &state, RBIM &cov) const { state = state_; cov = cov_; }
  const std::vector<double> &finalLogLikelihood() const { return ll_; }
  int64_t finalUtime(int s) const { return utime_[(size_t) s]; }   // batch-level time at which segment s ended

private:
  RBIS state_;
  RBIM cov_;
  std::vector<double> ll_;
  std::vector<int64_t> utime_;
  std::vector<uint8_t> finished_;
};

}  // namespace segment_channels
}  // namespace MavStateEst
