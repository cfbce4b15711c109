// segment_messages.cpp -- what SegmentBatcher and SegmentStreamer hand to the handlers, recorded on the CPU (tests/test_segment_messages.py).
// A small set of logs is written with pronto_wire::LogWriter and replayed through both replayers with plain callbacks against the HOST
// stubs of the C ABI (generated from include/pronto_batch.h by tests/test_host_sanitizers.py: PB_DEVICE blocks are heap blocks).  Every
// batched message is printed in dispatch order -- channel, batch utime, every member of every column, masked columns included, numbers as
// hex floats -- followed by the integer members of Stats and finalUtime.  One trace per replayer and configuration; each must equal
// tests/golden/segment_messages/<name>.txt byte for byte.  Only the public API of the two classes is used.
//
// The fixture: a batch of 5 filters with 4 segments (column 4 never has one) of 6 / 9 / 12 / 11 ticks on different absolute time
// bases with jittered stamps.  Segment 1 ends at an end_timestamp (the batcher, which has none, reads a copy of the log cut there),
// segment 2 is opened at a start_timestamp, segment 3 has one tick in another file order and its force/torque channel stops early
// (readahead_cap is small).  Every log carries a foreign channel, sparse POSE_SCAN / VO_UPDATE (one with an estimate_status that is not
// valid), KVH messages with repeated packets, no new packet, a packet count that goes backwards, more new packets than max_packets
// and a single packet, a payload cut in half, and (segment 3, its last tick) a joint-state message with another joint list.
// The streamer's lines leave column 4 out: it never writes the columns behind its last segment, and what they hold is whatever the
// ring buffer's last use left there -- which buffer that was depends on the timing of its two threads.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pronto_amd/csrc/segment_batcher.hpp"
#include "../../pronto_amd/csrc/segment_stream.hpp"

using namespace MavStateEst;

static const char *BOT_CORE_LCM = R"(package bot_core;
struct ins_t { int64_t utime; int64_t device_time; double gyro[3]; double mag[3]; double accel[3]; double quat[4]; double pressure; double rel_alt; }
struct joint_state_t { int64_t utime; int16_t num_joints; string joint_name[num_joints]; float joint_position[num_joints];
  float joint_velocity[num_joints]; float joint_effort[num_joints]; }
struct six_axis_force_torque_t { int64_t utime; double force[3]; double moment[3]; }
struct six_axis_force_torque_array_t { int64_t utime; int32_t num_sensors; string names[num_sensors]; six_axis_force_torque_t sensors[num_sensors]; }
struct pose_t { int64_t utime; double pos[3]; double vel[3]; double orientation[4]; double rotation_rate[3]; double accel[3]; }
struct kvh_raw_imu_t { int64_t utime; int64_t packet_count; double delta_rotation[3]; double linear_acceleration[3]; }
struct kvh_raw_imu_batch_t { int64_t utime; int32_t num_packets; kvh_raw_imu_t raw_imu[num_packets]; }
)";

static const int B = 5, MAX_PACKETS = 2;

struct LogSpec {
  int seg, ticks;
  int64_t base;
  int swap_tick = -1;      // force/torque and joint state in the other file order in this tick
  int ft_stops = 1 << 30;  // no force/torque message from this tick on
  int other_joints = -1;   // the joint-state message of this tick names other joints
  int64_t cut = 0;         // > 0: events stamped at or after it are left out (what an end_timestamp does)
};

static uint64_t rng_state;
static int64_t jitter()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (int64_t) ((rng_state >> 33) % 8) * 25;
}
static int64_t tick_time(const LogSpec &sp, int k) { return sp.base + (int64_t) (k + 1) * 2000; }

// numbers with short hex-float forms: signed powers of two from 1/8 to 16 (exact as float, too), shifted from segment to segment
static double val(int seg, int k, int i)
{
  const int v = seg * 5 + k * 3 + i;
  return (v % 3 == 0 ? -1.0 : 1.0) * (double) (1 << (v * 7 % 8)) * 0.125;
}

static void write_log(const pronto_wire::Schema &schema, const std::string &path, const LogSpec &sp)
{
  const std::vector<std::string> names = { "l_leg_kny", "r_leg_kny" }, others = { "l_arm_elx", "r_arm_elx" };
  pronto_wire::LogWriter log(path);
  rng_state = 0x5E67ULL + (uint64_t) sp.seg;
  auto put = [&](int64_t stamp, const char *channel, const std::vector<uint8_t> &buf) {
    if (sp.cut > 0 && stamp >= sp.cut) return;
    log.write(stamp, channel, buf);
  };
  int64_t newest = 100 + 50 * sp.seg;   // KVH packet count of the newest packet
  for (int k = 0; k < sp.ticks; k++) {
    const int64_t t = tick_time(sp, k) + jitter();
    const bool halved = k == 5 + sp.seg;   // this tick's IMU payloads are cut in half
    {
      pronto_wire::Writer w;
      w.u64(schema.fingerprint("bot_core.ins_t"));
      w.i64(t); w.i64(t + 17);
      for (int i = 0; i < 15; i++) w.f64(val(sp.seg, k, i));
      if (halved) w.buf.resize(w.buf.size() / 2);
      put(t, "IMU", w.buf);
    }
    {
      // raw_imu[0] is the newest packet; by default 3 packets of which 2 are new
      const int ks = k - sp.seg;   // (the special messages come at other ticks in every segment)
      int np = 3;
      if (ks == 2) newest += 0;                      // no new packet
      else if (ks == 4) newest = 20 + sp.seg;       // the packet count goes backwards
      else if (ks == 6) { newest += 4; np = 4; }     // more new packets than MAX_PACKETS
      else if (ks == 8) { newest += 1; np = 1; }     // one packet: no raw_dt without atlas_filter
      else newest += 2;
      pronto_wire::Writer q;
      q.u64(schema.fingerprint("bot_core.kvh_raw_imu_batch_t"));
      q.i64(t + 10); q.i32(np);
      for (int j = 0; j < np; j++) {
        q.i64(t - 1000 * j - (j ? jitter() : 0)); q.i64(newest - j);
        for (int i = 0; i < 6; i++) q.f64(val(sp.seg, k, 10 * j + i));
      }
      if (halved) q.buf.resize(q.buf.size() / 2);
      put(t + 10, "ATLAS_IMU_BATCH", q.buf);
    }
    if (k % 5 == 3) put(t + 50, "SOMETHING_ELSE", std::vector<uint8_t>(13, 0x5A));
    pronto_wire::Writer f;
    f.u64(schema.fingerprint("bot_core.six_axis_force_torque_array_t"));
    f.i64(t + 100); f.i32(2); f.str("l_foot"); f.str("r_foot");
    for (int s = 0; s < 2; s++) { f.i64(t + 100); for (int i = 0; i < 6; i++) f.f64(val(sp.seg, k, 40 + 6 * s + i)); }
    pronto_wire::Writer j;
    j.u64(schema.fingerprint("bot_core.joint_state_t"));
    j.i64(t + 300); j.i16((int16_t) names.size());
    for (const auto &nm : (k == sp.other_joints ? others : names)) j.str(nm);
    for (int r = 0; r < 3; r++)
      for (size_t i = 0; i < names.size(); i++) j.f32((float) val(sp.seg, k, 60 + 2 * r + (int) i));
    if (k == sp.swap_tick) {
      put(t + 100, "JOINT_STATE", j.buf);
      put(t + 300, "FORCE_TORQUE", f.buf);
    } else {
      if (k < sp.ft_stops) put(t + 100, "FORCE_TORQUE", f.buf);
      put(t + 300, "JOINT_STATE", j.buf);
    }
    if (k % 3 == 2) {
      pronto_wire::Writer p;
      p.u64(schema.fingerprint("bot_core.pose_t"));
      p.i64(t + 500);
      for (int i = 0; i < 16; i++) p.f64(val(sp.seg, k, 80 + i));
      put(t + 500, "POSE_SCAN", p.buf);
      pronto_wire::update_t u;
      u.timestamp = t + 600; u.prev_timestamp = t - 9400 + jitter();
      for (int i = 0; i < 3; i++) u.translation[i] = val(sp.seg, k, 100 + i);
      for (int i = 0; i < 4; i++) u.rotation[i] = val(sp.seg, k, 110 + i);
      u.estimate_status = k % 6 == 5 && sp.seg % 2 == 1 ? (int) pronto_wire::update_t::ESTIMATE_VALID + 1 : (int) pronto_wire::update_t::ESTIMATE_VALID;
      std::vector<uint8_t> ub;
      u.encode(ub);
      put(t + 600, "VO_UPDATE", ub);
    }
  }
}

// ---- the trace: one line per batched message: channel, batch utime, scalar members, the names of the per-column members, then the columns ----
static FILE *out = nullptr;
static int columns = B;   // columns a line carries (the rest: " ; -")
static void hex(const double *p, int rows, int s)
{
  fprintf(out, " ");
  for (int i = 0; i < rows; i++) fprintf(out, "%s%a", i ? "," : "", p[(size_t) i * B + s]);
}
static void hexf(const float *p, int rows, int s)
{
  fprintf(out, " ");
  for (int i = 0; i < rows; i++) fprintf(out, "%s%a", i ? "," : "", (double) p[(size_t) i * B + s]);
}
static void end_line()
{
  for (int s = columns; s < B; s++) fprintf(out, " ; -");
  fprintf(out, "\n");
}
static void on_ins(const msgs::ins_t *m)
{
  fprintf(out, "IMU %lld members=valid,gyro,accel", (long long) m->utime);
  for (int s = 0; s < columns; s++) {
    fprintf(out, " ; %d", (int) m->valid[s]);
    hex(m->gyro.p, 3, s);
    hex(m->accel.p, 3, s);
  }
  end_line();
}
static void on_kvh(const msgs::kvh_raw_imu_segments_t *m)
{
  fprintf(out, "ATLAS_IMU_BATCH %lld max_new=%d members=valid,n_new,utimes,new_accel,delta_rotation,raw_dt", (long long) m->utime, m->max_new);
  for (int s = 0; s < columns; s++) {
    fprintf(out, " ; %d %d %lld", (int) m->valid[s], (int) m->n_new[s], (long long) m->utimes[s]);
    hex(m->new_accel, 3 * m->max_new, s);
    hex(m->delta_rotation, 3, s);
    hex(m->raw_dt, 1, s);
  }
  end_line();
}
static void on_joints(const msgs::joint_state_t *m)
{
  fprintf(out, "JOINT_STATE %lld members=valid,utimes,joint_position,joint_velocity,joint_effort joint_name=", (long long) m->utime);
  for (size_t i = 0; i < m->joint_name.size(); i++) fprintf(out, "%s%s", i ? "," : "", m->joint_name[i].c_str());
  const int n = (int) m->joint_name.size();
  for (int s = 0; s < columns; s++) {
    fprintf(out, " ; %d %lld", (int) m->valid[s], (long long) m->utimes[s]);
    hexf(m->joint_position, n, s);
    hexf(m->joint_velocity, n, s);
    hexf(m->joint_effort, n, s);
  }
  end_line();
}
static void on_pose(const msgs::pose_t *m)
{
  fprintf(out, "POSE_SCAN %lld members=valid,pos,vel,orientation", (long long) m->utime);
  for (int s = 0; s < columns; s++) {
    fprintf(out, " ; %d", (int) m->valid[s]);
    hex(m->pos.p, 3, s);
    hex(m->vel.p, 3, s);
    hex(m->orientation.p, 4, s);
  }
  end_line();
}
static void on_update(const msgs::update_t *m)
{
  fprintf(out, "VO_UPDATE %lld prev_timestamp=%lld members=valid,translation,rotation", (long long) m->timestamp, (long long) m->prev_timestamp);
  for (int s = 0; s < columns; s++) {
    fprintf(out, " ; %d", (int) m->estimate_valid[s]);
    hex(m->translation.p, 3, s);
    hex(m->rotation.p, 4, s);
  }
  end_line();
}

enum Imu { INS, KVH_FILTER, KVH_NEWEST };
static const char *IMU_NAME[] = { "ins", "kvh_filter", "kvh_newest" };

template <class R>
static void subscribe_common(R &r, const pronto_wire::Schema &schema, Imu imu)
{
  if (imu == INS) r.subscribeIns("IMU", &schema, "bot_core.ins_t", on_ins);
  else r.subscribeKvhBatch("ATLAS_IMU_BATCH", &schema, "bot_core.kvh_raw_imu_batch_t", imu == KVH_FILTER, MAX_PACKETS, on_kvh);
  r.subscribeJointState("JOINT_STATE", &schema, "bot_core.joint_state_t", on_joints);
  r.subscribePose("POSE_SCAN", &schema, "bot_core.pose_t", on_pose);
  r.subscribeUpdate("VO_UPDATE", on_update);
}
template <class R>
static void print_stats(const R &r)
{
  const auto &st = r.stats;
  fprintf(out, "stats batches=%lld segment_messages=%lld ragged=%lld order_violations=%lld undecodable=%lld max_skew_us=%lld readahead_capped=%lld\n",
          (long long) st.batches, (long long) st.segment_messages, (long long) st.ragged, (long long) st.order_violations, (long long) st.undecodable,
          (long long) st.max_skew_us, (long long) st.readahead_capped);
  fprintf(out, "per_channel");
  for (const auto &kv : st.per_channel) fprintf(out, " %s=%lld", kv.first.c_str(), (long long) kv.second);
  fprintf(out, "\nfinal_utime");
  for (int s = 0; s < B; s++) fprintf(out, " %lld", (long long) r.finalUtime(s));
  fprintf(out, "\n");
}
static void open_trace(const std::string &dir, const std::string &name)
{
  out = fopen((dir + "/" + name + ".txt").c_str(), "w");
  if (!out) { printf("cannot write %s/%s.txt\n", dir.c_str(), name.c_str()); exit(2); }
}

int main(int argc, char **argv)
{
  if (argc < 2) { printf("usage: segment_messages <output directory>\n"); return 2; }
  const std::string dir = argv[1];
  pronto_wire::Schema schema;
  std::string err;
  if (!schema.parse(BOT_CORE_LCM, &err)) { printf("schema: %s\n", err.c_str()); return 2; }

  LogSpec sp[4] = { { 0, 6, 1000000000LL }, { 1, 12, 5000000123LL }, { 2, 15, 2000000777LL }, { 3, 11, 9000000001LL } };
  const int64_t end1 = tick_time(sp[1], 9) - 500, start2 = tick_time(sp[2], 3) - 500;
  sp[3].other_joints = 10;
  sp[3].swap_tick = 1;
  sp[3].ft_stops = 3;
  std::string path[4], cut1 = dir + "/seg1_cut.lcmlog";
  for (int s = 0; s < 4; s++) {
    path[s] = dir + "/seg" + std::to_string(s) + ".lcmlog";
    write_log(schema, path[s], sp[s]);
  }
  LogSpec c1 = sp[1];
  c1.cut = end1;
  write_log(schema, cut1, c1);

  BotParam param;
  param.set("state_estimator.utime_history_span", "1000000");
  param.set("state_estimator.history_slots", "0");
  RBIS x0(15, B);
  RBIM P0(15, B);
  const size_t cap = 16;   // (the batcher reads segment 2's log from its start: the events in front of start_timestamp count)
  for (Imu imu : { INS, KVH_FILTER, KVH_NEWEST }) {
    {
      MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
      SegmentBatcher batch(&est);
      batch.readahead_cap = cap;
      if (!batch.addSegment(path[0]) || !batch.addSegment(cut1) || !batch.addSegment(path[2], start2) || !batch.addSegment(path[3])) return 2;
      subscribe_common(batch, schema, imu);
      batch.subscribeForceTorque("FORCE_TORQUE", &schema, "bot_core.six_axis_force_torque_array_t", [](const msgs::six_axis_force_torque_array_t *m) {
        fprintf(out, "FORCE_TORQUE %lld members=force_z", (long long) m->utime);
        for (int s = 0; s < B; s++) { fprintf(out, " ;"); hex(m->force_z.p, 2, s); }
        fprintf(out, "\n");
      });
      columns = B;
      open_trace(dir, std::string("batcher_") + IMU_NAME[imu]);
      batch.run();
      print_stats(batch);
      fclose(out);
    }
    struct Run { const char *name; int max_slots; uint64_t budget; };
    for (const Run &rn : { Run{ "slots1", 1, 0 }, Run{ "slots7", 7, 0 }, Run{ "slots96", 96, 0 }, Run{ "budget", 96, 2048 } }) {
      // (slots96 with every IMU channel, against the batcher; the other chunkings with ins_t, the KVH de-duplication state across chunk borders with slots7)
      const bool plain96 = rn.max_slots == 96 && rn.budget == 0;
      if (!plain96 && (imu == KVH_FILTER) != (rn.max_slots == 7)) continue;
      if (!plain96 && imu == KVH_NEWEST) continue;
      MavStateEstimator est(new RBISResetUpdate(x0, P0, RBISUpdateInterface::reset, 0), &param, 0);
      SegmentStreamer stream(&est);
      stream.readahead_cap = cap;
      stream.max_slots = rn.max_slots;
      if (rn.budget) stream.chunk_budget_bytes = rn.budget;   // (a block of 5 columns is 256 bytes: 8 batched messages per chunk)
      if (!stream.addSegment(path[0]) || !stream.addSegment(path[1], 0, end1) || !stream.addSegment(path[2], start2) || !stream.addSegment(path[3])) return 2;
      subscribe_common(stream, schema, imu);
      // (the streamer's force/torque callback has no message time: the line carries none)
      stream.subscribeForceTorque("FORCE_TORQUE", &schema, "bot_core.six_axis_force_torque_array_t", [](const float *abs_force_z) {
        fprintf(out, "FORCE_TORQUE - members=force_z");
        for (int s = 0; s < columns; s++) { fprintf(out, " ;"); hexf(abs_force_z, 2, s); }
        end_line();
      });
      columns = stream.segments();
      open_trace(dir, std::string("streamer_") + IMU_NAME[imu] + "_" + rn.name);
      stream.run();
      print_stats(stream);
      fprintf(out, "chunks=%lld uploaded_bytes=%llu\n", (long long) stream.stats.chunks, (unsigned long long) stream.stats.uploaded_bytes);
      fclose(out);
    }
  }
  for (int s = 0; s < 4; s++) remove(path[s].c_str());
  remove(cut1.c_str());
  printf("PASS\n");
  return 0;
}
