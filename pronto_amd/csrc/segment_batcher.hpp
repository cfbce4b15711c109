// segment_batcher.hpp -- N independent log segments replayed as ONE batch: segment s feeds filter s.
//
// The reference's many-runs workload is a loop over recorded logs, one se-fusion process after the other
// (motion_estimate/scripts/se-batch-process.sh:17-26,58-59,70-74), each opened as "file://<log>?speed=..&start_timestamp=<t>"
// (state-estimator/src/mav_state_est/lcm_front_end.cpp:21-33: the log provider skips to the first event at or after t).  Here
// the N runs share every kernel launch: the k-th message of a channel in each segment becomes column s of ONE batched message
// ([rows][B] host blocks, filter index fastest) that is handed to the callback LCMFrontEnd::addSensor returns -- the same
// handlers, the same estimator, B = N filters.  LogPlayer (mav_state_est_batch.hpp) is the other case: one log for every filter.
//
// Alignment.  Messages are aligned BY INDEX per channel, and the channels are dispatched in the file order of the LEAD segment
// (the lowest-numbered segment that still has events).  That is exact for segments recorded by the same robot software -- the
// same channels at the same rates in the same interleaving -- which is what a set of runs of one robot, or N start offsets into
// one long log, are.  What is checked instead of assumed:
//   * order_violations   a segment's own file order differs from the lead's (its k-th message of channel C was not the next
//                        subscribed event in its log): the filter then sees its updates in the lead's order, not its own;
//   * max_skew_us        largest difference between a segment's message time (relative to its first dispatched message) and the
//                        lead's for the same batched message.
// Time.  A batched message carries the LEAD's time, relative to the lead's first message, on the time base of the first segment (it
// orders the update in the estimator's history and stays continuous when the lead changes).  Every filter's own time
// stamp travels beside it where the arithmetic reads one: the leg odometry (msgs::joint_state_t::utimes -> per-filter elapsed
// time, 30 ms reset, contact-classifier clocks: pb_legodo_set_message_times).  InsHandler::processMessage integrates with the
// configured timestep_dt like the reference (sensor_handlers.cpp:96-131), so it needs none.
// Ragged ends.  A segment that runs out of messages on a channel gets valid = 0 in that channel's batched messages from then on:
// its measurements are masked and its IMU step is taken with dt = 0 on its own last sample.  The RESULT of a run is its head at the
// end of ITS log: the moment a segment has no event left, its filter's head is read into finalState() / finalLogLikelihood()
// (one pb_get_head per run of segments that end together: with equal-length segments one call for the whole batch).  The
// filter idles in the batch afterwards; an idle step keeps pose, velocity, biases and covariance but re-derives the
// angular-velocity / acceleration entries from its last sample, so the estimator's own head is NOT the result of a finished run.
//
// Smoothing.  enableSmoothing() before run() makes the batch the reference's "-S" run of every log (lcm_front_end.cpp:168-203,
// mav_state_est.cpp:98-189): a checkpoint slot is taken out of the estimator's pool for the TERMINAL posteriors, and finalize() copies
// the head of the segments that end into it (pb_slot_select, on the device), so that it holds every segment's posterior at the end of
// its own log.  The batcher also keeps every batched IMU message's per-segment validity and time on the host.  smooth(dt, sink) then
// runs the estimator's ragged-aware EKFSmoothBackwardsPass (terminal slot as the newest step's "next", pb_smooth_step_masked on the
// ticks some segment sat out) and calls sink(step, slot, emit, utimes) once per batched IMU message, newest first: `slot` holds the
// smoothed posteriors of that tick until the next call; emit[s] = 1 exactly where it is one of segment s's smoothed posteriors -- s had
// an INS update at this tick and has a later one in the history -- so segment s receives its own INS update count - 1 of them, newest
// first, as a single-segment pass over its log would; utimes[s] = segment s's own message time; step = the index of this IMU message in
// every segment's own log (messages are aligned by index per channel).  The history must keep the whole log (utime_history_span,
// history_slots).  INS updates are matched to batched IMU messages by batch time; smooth() returns -1 when two messages share one.
//
// Host side only; every batched array lives in page-locked memory (pb_host_alloc) so that the library's double-buffered staging
// copies run as DMA.  Decoding goes through the run-time .lcm schema (lcm_schema.hpp): the bot_core definitions are the caller's.
#pragma once

#include <chrono>
#include <deque>

#include "segment_channels.hpp"

namespace MavStateEst {

class SegmentBatcher {
public:
  struct Stats {
    int64_t batches = 0;            // batched messages dispatched
    int64_t segment_messages = 0;   // per-segment messages they carried
    int64_t ragged = 0;             // columns without a message (segment ended)
    int64_t order_violations = 0, undecodable = 0, max_skew_us = 0;
    int64_t readahead_capped = 0;   // ticks in which a segment read `readahead_cap` events ahead without finding the channel's next message
    std::map<std::string, int64_t> per_channel;
    // where run() spent its wall-clock time, seconds: finding the lead (serial; includes its read-ahead), the segments' reads +
    // decodes (parallel), book-keeping (serial), assembling the batched arrays + the handler call (parallel loop + one enqueue),
    // the read-ahead of the next messages (parallel), reading finished runs' heads
    double t_lead = 0, t_pull = 0, t_book = 0, t_dispatch = 0, t_fill = 0, t_final = 0;
    double t_handler = 0, t_upload = 0;   // of t_dispatch: inside the handlers' callbacks (host passes, enqueues), the joint blocks' DMA

  };
  Stats stats;
  size_t readahead_cap = 4096;

  explicit SegmentBatcher(MavStateEstimator *est) : est_(est), B_(est->B), results_(est->n, est->B) {}
  ~SegmentBatcher()
  {
    est_->flushPending();   // (an update the estimator is holding back may still read the device blocks)
    pb_sync(est_->ctx);
    if (terminal_ >= 0) est_->releaseSlot(terminal_);
    for (void *p : pinned_) pb_host_free(est_->ctx, p);
    for (void *p : device_) pb_free(est_->ctx, p);
  }
  SegmentBatcher(const SegmentBatcher &) = delete;
  SegmentBatcher &operator=(const SegmentBatcher &) = delete;

  template <class F>
  void timed(double &acc, F &&f)
  {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  // segment s = filter s, in the order added; false: the file cannot be opened or the batch is full
  bool addSegment(const std::string &path, int64_t start_timestamp = 0)
  {
    if ((int) segs_.size() >= B_) return false;
    auto sg = std::unique_ptr<Seg>(new Seg(path, start_timestamp));
    if (!sg->rd.good()) return false;
    segs_.push_back(std::move(sg));
    return true;
  }
  int segments() const { return (int) segs_.size(); }

  // Before run(): keep what smooth() needs (see the head of this file).  false: the estimator has no free checkpoint slot.
  bool enableSmoothing()
  {
    if (terminal_ >= 0) return true;
    est_->flushPending();
    terminal_ = est_->reserveSlot();
    if (terminal_ < 0) {
      fprintf(stderr, "SegmentBatcher::enableSmoothing: no free checkpoint slot (state_estimator.history_slots)\n");
      return false;
    }
    // (every column holds a posterior from the start: a segment never added, or one that never ends, keeps its initial state)
    if (pb_state_save(est_->ctx, terminal_) != PB_OK) {
      fprintf(stderr, "SegmentBatcher: %s\n", pb_last_error(est_->ctx));
      est_->releaseSlot(terminal_);
      terminal_ = -1;
      return false;
    }
    return true;
  }
  // The smoothed posteriors of every segment, newest first (see the head of this file).  Returns the number of sink calls (batched IMU
  // messages smoothed), -1 on an error (smoothing not enabled, or the estimator's pass failed).
  int smooth(double dt, std::function<void(int segment_step_base, int slot, const uint8_t *emit_host, const int64_t *utime_host)> sink)
  {
    if (terminal_ < 0) {
      fprintf(stderr, "SegmentBatcher::smooth: enableSmoothing() was not called before run()\n");
      return -1;
    }
    if (terminal_failed_) {
      fprintf(stderr, "SegmentBatcher::smooth: a segment's final posterior could not be kept (see the error of finalize)\n");
      return -1;
    }
    est_->flushPending();
    // batched IMU message by its batch-level time (one message per time: the pass names an INS update by its time)
    std::map<int64_t, int> tick_of;
    for (int t = 0; t < (int) imu_tick_utime_.size(); t++)
      if (!tick_of.emplace(imu_tick_utime_[(size_t) t], t).second) {
        fprintf(stderr, "SegmentBatcher::smooth: two batched IMU messages at batch time %lld\n", (long long) imu_tick_utime_[(size_t) t]);
        return -1;
      }
    // each segment's last INS UPDATE in the history (the handler may have made no step of an IMU message: downsampling)
    std::vector<int> last((size_t) B_, -1);
    for (auto u = est_->history.updateMap.begin(); u != est_->unprocessed_updates_start; ++u) {
      if (u->second->sensor_id != RBISUpdateInterface::ins) continue;
      auto it = tick_of.find(u->first);
      if (it == tick_of.end()) {
        fprintf(stderr, "SegmentBatcher::smooth: an INS update at %lld that no batched IMU message made\n", (long long) u->first);
        return -1;
      }
      for (int s = 0; s < B_; s++)
        if (imu_valid_[(size_t) it->second * B_ + s]) last[(size_t) s] = std::max(last[(size_t) s], it->second);
    }
    std::vector<uint8_t> emit((size_t) B_, 0);
    int calls = 0;
    bool lost = false;
    const int steps = est_->EKFSmoothBackwardsPass(dt, terminal_, [&](int64_t utime, int slot, const uint8_t *, int) {
      auto it = tick_of.find(utime);   // (found: every INS update of the history was matched above)
      const int t = it == tick_of.end() ? -1 : it->second;
      lost = lost || t < 0;
      if (t < 0) return;
      for (int s = 0; s < B_; s++) emit[(size_t) s] = imu_valid_[(size_t) t * B_ + s] && t < last[(size_t) s];
      sink(t, slot, emit.data(), &imu_utime_[(size_t) t * B_]);
      calls++;
    });
    return steps < 0 || lost ? -1 : calls;
  }

  // ---- typed subscriptions: channel -> the callback FrontEnd::addSensor returned ----
  // What a channel reads of its wire type and the record it is decoded into are segment_channels.hpp's; here the records of a batched message's
  // columns are scattered into the channel's page-locked block.  A column without a message keeps what the block held, masked -- except where noted.
  // bot_core::ins_t by field name (utime, gyro[3], accel[3]): InsHandler::processMessage
  void subscribeIns(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                    std::function<void(const msgs::ins_t *)> cb)
  {
    typedef segment_channels::InsChannel C;
    auto ch = std::make_shared<C>(schema, type, "SegmentBatcher");
    Chan c;
    c.decode = record_decoder(ch, C::BYTES);
    uint8_t *blk = block(C::BYTES);
    c.dispatch = [this, cb, blk](const std::vector<const Rec *> &col, int64_t utime) {
      uint8_t *valid = rows<uint8_t>(blk, C::VALID);
      PB_SHIM_PARALLEL_FOR
      for (int s = 0; s < B_; s++) {
        const Rec *r = col[(size_t) s];
        valid[s] = r != nullptr;
        if (r) put<double>(blk, C::GYRO, 6, r->bytes.data(), s);   // (a filter without a message idles on its own last sample)
      }
      const msgs::ins_t m = C::message(utime, blk, (size_t) B_, PB_HOST);
      keep_imu_tick(col, valid, utime);
      timed(stats.t_handler, [&]() { cb(&m); });
    };
    chans_[channel] = std::move(c);
  }
  // bot_core::kvh_raw_imu_batch_t: the reference's Atlas IMU channel (fusion.cpp:161-163 -> InsHandler::processMessageAtlas,
  // sensor_handlers.cpp:165-252) for N independent logs -> InsHandler::processMessageAtlasSegments.  atlas_filter = the handler's;
  // max_packets = rows of the new-packet block (more NEW packets than that are clamped).  A column without a message has utimes = 0.
  void subscribeKvhBatch(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type, bool atlas_filter, int max_packets,
                         std::function<void(const msgs::kvh_raw_imu_segments_t *)> cb)
  {
    typedef segment_channels::KvhChannel C;
    auto ch = std::make_shared<C>(schema, type, atlas_filter, max_packets, "SegmentBatcher");
    Chan c;
    c.decode = record_decoder(ch, ch->BYTES);
    uint8_t *blk = block(ch->BYTES);
    std::fill_n(rows<double>(blk, ch->RAW_DT), (size_t) B_, 1.0);
    c.dispatch = [this, cb, ch, blk](const std::vector<const Rec *> &col, int64_t utime) {
      int32_t *n_new = rows<int32_t>(blk, ch->N_NEW);
      uint8_t *valid = rows<uint8_t>(blk, ch->VALID);
      int64_t *ut = rows<int64_t>(blk, ch->UTIME);
      PB_SHIM_PARALLEL_FOR
      for (int s = 0; s < B_; s++) {
        const Rec *r = col[(size_t) s];
        const int nn = r ? (int) *segment_channels::member<int32_t>(r->bytes.data(), ch->N_NEW) : 0;
        n_new[s] = nn;
        valid[s] = nn > 0;
        ut[s] = r ? r->utime : 0;
        if (nn <= 0) continue;   // (no message, or no new packet: the filter idles; its arrays keep their last values)
        put<double>(blk, ch->ACCEL, (size_t) 3 * nn, r->bytes.data(), s);
        put<double>(blk, ch->DELTA_ROTATION, 3, r->bytes.data(), s);
        put<double>(blk, ch->RAW_DT, 1, r->bytes.data(), s);
      }
      const msgs::kvh_raw_imu_segments_t m = ch->message(utime, blk, (size_t) B_, PB_HOST);
      keep_imu_tick(col, valid, utime);
      timed(stats.t_handler, [&]() { cb(&m); });
    };
    chans_[channel] = std::move(c);
  }
  // bot_core::joint_state_t (utime, joint_name[], joint_position[], joint_velocity[], joint_effort[]): LegOdoHandler::processMessage.
  // Every segment's list is held to the LEAD's of the same batched message; a column with another list is masked and counted as undecodable.
  void subscribeJointState(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                           std::function<void(const msgs::joint_state_t *)> cb)
  {
    typedef segment_channels::JointStateChannel C;
    auto ch = std::make_shared<C>(schema, type, "SegmentBatcher");
    Chan c;
    c.decode = [ch](const pronto_wire::LogEvent &ev, Rec &r, Stream &st) {
      const std::vector<std::string> *fresh = nullptr;
      if (!ch->open(ev.data.data(), ev.data.size(), st, &fresh)) return false;
      if (fresh) st.names = std::make_shared<const std::vector<std::string>>(*fresh);   // a new joint list (normally: the first message of the segment)
      const C::Layout lay(st.names->size());
      r.bytes.resize(lay.BYTES);
      r.names = st.names;
      r.names_hash = st.names_hash;
      return ch->read(ev.data.data(), st, lay, r.bytes.data(), r.utime);
    };
    auto st = std::make_shared<JointBlocks>();
    c.dispatch = [this, cb, st](const std::vector<const Rec *> &col, int64_t utime) {
      const Rec *lead = nullptr;
      for (const Rec *r : col)
        if (r) { lead = r; break; }
      if (lead == nullptr) return;
      const size_t n = lead->names->size(), B = (size_t) B_;
      const C::Layout lay(n);
      if (st->rows != n || st->blk == nullptr) {   // first message (or a new joint list): size the page-locked block and its float part in HBM
        st->rows = n;
        st->blk = block(lay.BYTES);
        void *d = nullptr;
        if (pb_malloc(est_->ctx, sizeof(float) * 3 * n * B, &d) != PB_OK) {
          fprintf(stderr, "SegmentBatcher: %s\n", pb_last_error(est_->ctx));
          exit(1);
        }
        st->d_jp = (float *) d;
        device_.push_back(d);
      }
      uint8_t *blk = st->blk, *valid = rows<uint8_t>(blk, lay.VALID);
      int64_t *ut = rows<int64_t>(blk, lay.UTIME);
      int64_t mismatched = 0;
      PB_SHIM_PARALLEL_FOR_SUM(mismatched)
      for (int s = 0; s < B_; s++) {
        const Rec *r = col[(size_t) s];
        // one robot model for the batch: the same joints in the same order (compared by the hash of the name list, made where the
        // list was decoded: 30 string compares per segment and message were a third of this loop)
        const bool ok = r != nullptr && r->names_hash == lead->names_hash && r->names->size() == n;
        if (r != nullptr && !ok) mismatched++;
        valid[s] = ok;
        ut[s] = ok ? r->utime : 0;
        if (ok) put<float>(blk, lay.POSITION, 3 * n, r->bytes.data(), s);   // (else the block keeps this filter's last message; it is masked)
      }
      stats.undecodable += mismatched;
      // The joint block goes to HBM here (one DMA from page-locked memory) and the handler gets a DEVICE message: with the IMU
      // block coming from the host, the IMU + joint-state pair then runs as ONE kernel (pb_step_legodo_joints takes at most one
      // of its two input groups from the host).  The previous message's pair kernel has been enqueued by now and the copy is
      // stream-ordered behind it, so one device block is enough.  (The call takes ~300 us at 4096 segments where the DMA of a busy
      // device takes 25: a copy on a second stream into alternating blocks, waiting for nothing but itself, took the same -- the
      // device idles between ticks in this host-bound replay and every burst pays its wake-up.)
      int urc = PB_OK;
      timed(stats.t_upload, [&]() { urc = pb_memcpy_h2d(est_->ctx, st->d_jp, rows<float>(blk, lay.POSITION), sizeof(float) * 3 * n * B); });
      if (urc != PB_OK) {
        fprintf(stderr, "SegmentBatcher: %s\n", pb_last_error(est_->ctx));
        return;
      }
      const msgs::joint_state_t m = C::message(utime, *lead->names, lay, B, st->d_jp, PB_DEVICE, blk, PB_HOST);
      timed(stats.t_handler, [&]() { cb(&m); });
    };
    chans_[channel] = std::move(c);
  }
  // bot_core::six_axis_force_torque_array_t (sensors[].force[3]; sensors 0 / 1 = left / right foot): LegOdoHandler::forceTorqueHandler,
  // with the signed force z of the two feet as doubles, [2][B]
  void subscribeForceTorque(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                            std::function<void(const msgs::six_axis_force_torque_array_t *)> cb)
  {
    auto ch = std::make_shared<segment_channels::ForceTorqueChannel>(schema, type, "SegmentBatcher");
    Chan c;
    c.decode = [ch](const pronto_wire::LogEvent &ev, Rec &r, Stream &st) {
      r.bytes.resize(2 * sizeof(double));
      return ch->decode(ev.data.data(), ev.data.size(), st, (double *) r.bytes.data(), r.utime);
    };
    uint8_t *blk = block(2 * sizeof(double));
    c.dispatch = [this, cb, blk](const std::vector<const Rec *> &col, int64_t utime) {
      PB_SHIM_PARALLEL_FOR
      for (int s = 0; s < B_; s++)
        if (col[(size_t) s]) put<double>(blk, 0, 2, col[(size_t) s]->bytes.data(), s);   // (the handler keeps the LAST force/torque message, per filter: a missing one changes nothing)
      msgs::six_axis_force_torque_array_t m{ utime, BatchArray((const double *) blk, PB_HOST) };
      timed(stats.t_handler, [&]() { cb(&m); });
    };
    chans_[channel] = std::move(c);
  }
  // pronto::update_t (pronto_wire.hpp): FovisHandler::processMessage.  timestamp / prev_timestamp are the lead's.  A column without a
  // message is blank.
  void subscribeUpdate(const std::string &channel, std::function<void(const msgs::update_t *)> cb)
  {
    typedef segment_channels::UpdateChannel C;
    Chan c;
    c.decode = [](const pronto_wire::LogEvent &ev, Rec &r, Stream &) {
      r.bytes.resize(C::BYTES);
      return C::decode(ev.data.data(), ev.data.size(), r.bytes.data(), r.utime, &r.prev_behind);
    };
    uint8_t *blk = block(C::BYTES);
    c.dispatch = [this, cb, blk](const std::vector<const Rec *> &col, int64_t utime) {
      uint8_t none[C::BYTES];
      C::blank(none);
      const Rec *lead = nullptr;
      for (int s = 0; s < B_; s++) {
        const Rec *r = col[(size_t) s];
        if (r && !lead) lead = r;
        put<double>(blk, C::TRANSLATION, 7, r ? r->bytes.data() : none, s);
        put<uint8_t>(blk, C::VALID, 1, r ? r->bytes.data() : none, s);
      }
      if (lead == nullptr) return;
      const msgs::update_t m = C::message(utime, lead->prev_behind, blk, (size_t) B_);
      cb(&m);
    };
    chans_[channel] = std::move(c);
  }
  // bot_core::pose_t (utime, pos[3], vel[3], orientation[4]): ScanMatcherHandler::processMessage.  A column without a message is blank.
  void subscribePose(const std::string &channel, const pronto_wire::Schema *schema, const std::string &type,
                     std::function<void(const msgs::pose_t *)> cb)
  {
    typedef segment_channels::PoseChannel C;
    auto ch = std::make_shared<C>(schema, type, "SegmentBatcher");
    Chan c;
    c.decode = record_decoder(ch, C::BYTES);
    uint8_t *blk = block(C::BYTES);
    c.dispatch = [this, cb, blk](const std::vector<const Rec *> &col, int64_t utime) {
      uint8_t none[C::BYTES];
      C::blank(none);
      PB_SHIM_PARALLEL_FOR
      for (int s = 0; s < B_; s++) {
        const uint8_t *rec = col[(size_t) s] ? col[(size_t) s]->bytes.data() : none;
        put<double>(blk, C::POS, 10, rec, s);
        put<uint8_t>(blk, C::VALID, 1, rec, s);
      }
      const msgs::pose_t m = C::message(utime, blk, (size_t) B_);
      cb(&m);
    };
    chans_[channel] = std::move(c);
  }

  // Replays every segment to its end.  Returns the number of batched messages dispatched, or -1 when no segment was added.
  int64_t run()
  {
    if (segs_.empty()) return -1;
    // channels by index from here on: the per-event work is one name look-up, then deques of ints
    chan_list_.clear();
    chan_names_.clear();
    for (auto &kv : chans_) {
      kv.second.id = (int) chan_list_.size();
      chan_list_.push_back(&kv.second);
      chan_names_.push_back(kv.first);
    }
    for (auto &sg : segs_)
      if (sg->queue.size() != chan_list_.size()) {
        sg->queue.resize(chan_list_.size());
        sg->stream.resize(chan_list_.size());
      }
    std::vector<const Rec *> col((size_t) B_, nullptr);
    std::vector<Rec> held((size_t) B_);
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto lap = [&now](std::chrono::steady_clock::time_point &t, double &acc) {
      const auto t1 = now();
      acc += std::chrono::duration<double>(t1 - t).count();
      t = t1;
    };
    for (;;) {
      auto tick = now();
      // the lead: the first segment that still has a subscribed event; its next one names the channel of this batched message
      int lead = -1, channel = -1;
      for (int s = first_alive_; s < (int) segs_.size() && lead < 0; s++) {
        if (fill(*segs_[(size_t) s]) && !segs_[(size_t) s]->order.empty()) {
          lead = s;
          channel = segs_[(size_t) s]->order.front();
        } else if (s == first_alive_) {
          first_alive_++;   // (ended for good: not asked again)
        }
      }
      if (lead < 0) break;
      Chan &ch = *chan_list_[(size_t) channel];
      int64_t lead_rel = 0;
      std::fill(col.begin(), col.end(), nullptr);
      const int nseg = (int) segs_.size();
      lap(tick, stats.t_lead);
      // every segment reads and decodes its own log: independent work, one host thread per range of segments (-fopenmp)
      PB_SHIM_PARALLEL_FOR
      for (int s = lead; s < nseg; s++) got_[(size_t) s] = pull(*segs_[(size_t) s], channel, held[(size_t) s]);
      lap(tick, stats.t_pull);
      for (int s = lead; s < nseg; s++) {
        Seg &sg = *segs_[(size_t) s];
        if (!got_[(size_t) s]) {
          stats.ragged++;
          continue;
        }
        col[(size_t) s] = &held[(size_t) s];
        if (sg.t0 == INT64_MIN) sg.t0 = held[(size_t) s].utime;
        const int64_t rel = held[(size_t) s].utime - sg.t0;
        if (s == lead) {
          lead_rel = rel;
          if (base_ == INT64_MIN) base_ = sg.t0;   // the batch's time base: the first lead's first message
        } else {
          stats.max_skew_us = std::max<int64_t>(stats.max_skew_us, std::llabs(rel - lead_rel));
        }
        stats.segment_messages++;
      }
      stats.ragged += lead;   // (the segments in front of the lead have ended)
      lap(tick, stats.t_book);
      // batch-level time of this message: the lead's, relative to ITS first message, on the batch's base -- it stays continuous when
      // the lead changes (segments come from different recordings: their absolute times have nothing to do with each other)
      ch.dispatch(col, base_ + lead_rel);
      stats.batches++;
      stats.per_channel[chan_names_[(size_t) channel]]++;
      lap(tick, stats.t_dispatch);
      // segments whose log has no subscribed event left: their run is complete, keep its result.  (fill() is also the read-ahead
      // of the next message: in parallel over the segments)
      PB_SHIM_PARALLEL_FOR
      for (int s = 0; s < nseg; s++) got_[(size_t) s] = results_.finished(s) || fill(*segs_[(size_t) s]);
      lap(tick, stats.t_fill);
      int first = -1;
      for (int s = 0; s <= nseg; s++) {
        const bool ended = s < nseg && !results_.finished(s) && !got_[(size_t) s];
        if (ended && first < 0) first = s;
        if (!ended && first >= 0) {
          finalize(first, s - first);
          first = -1;
        }
      }
      lap(tick, stats.t_final);
    }
    for (const auto &sg : segs_) {
      stats.undecodable += sg->undecodable;
      stats.order_violations += sg->order_violations;
      stats.readahead_capped += sg->capped;
      sg->undecodable = sg->order_violations = sg->capped = 0;
    }
    return stats.batches;
  }

  // the head of every segment's filter at the end of ITS log (valid after run(); columns of segments never added are zero)
  void finalState(RBIS &state, RBIM &cov) const { results_.finalState(state, cov); }
  const std::vector<double> &finalLogLikelihood() const { return results_.finalLogLikelihood(); }
  int64_t finalUtime(int s) const { return results_.finalUtime(s); }   // batch-level time at which segment s ended

private:
  struct Stream : segment_channels::ChannelState {   // what one segment remembers about one channel ... and the joint list itself
    std::shared_ptr<const std::vector<std::string>> names;
  };
  // one decoded message: its time and its channel's record (segment_channels.hpp)
  struct Rec {
    int64_t utime = 0, prev_behind = 0;   // (update_t: prev_timestamp - timestamp)
    std::vector<uint8_t> bytes;
    std::shared_ptr<const std::vector<std::string>> names;   // joint state: shared by the messages of one stream, a joint list is decoded once
    uint64_t names_hash = 0;
  };
  struct Chan {
    std::function<bool(const pronto_wire::LogEvent &, Rec &, Stream &)> decode;
    std::function<void(const std::vector<const Rec *> &, int64_t)> dispatch;
    int id = -1;
  };
  struct JointBlocks {
    size_t rows = 0;
    uint8_t *blk = nullptr;   // page-locked assembly block ...
    float *d_jp = nullptr;    // ... and the copy of its float part in HBM
  };
  struct Seg {
    pronto_wire::LogReader rd;
    int64_t start_timestamp, t0 = INT64_MIN;
    bool eof = false;
    std::deque<int> order;                              // channels (index) of the decoded, not yet consumed events, in file order
    std::vector<std::deque<Rec>> queue;                 // ... and the events themselves, per channel
    std::vector<Stream> stream;
    int64_t undecodable = 0, order_violations = 0, capped = 0;      // (per segment: the segments are read by different host threads)
    Seg(const std::string &path, int64_t start) : rd(path), start_timestamp(start) {}
  };

  // reads ahead in the segment's log until one subscribed event is waiting (false: the log has ended and nothing is waiting)
  bool fill(Seg &sg)
  {
    while (sg.order.empty() && !sg.eof) read_one(sg);
    return !sg.order.empty();
  }
  void read_one(Seg &sg)
  {
    static thread_local pronto_wire::LogEvent ev;       // (its buffers are re-used from event to event)
    if (!sg.rd.next(ev)) {
      sg.eof = true;
      return;
    }
    if (ev.timestamp < sg.start_timestamp) return;      // "?start_timestamp=": lcm_front_end.cpp:21-33
    auto it = chans_.find(ev.channel);
    if (it == chans_.end()) return;
    const int id = it->second.id;
    Rec r;
    if (!it->second.decode(ev, r, sg.stream[(size_t) id])) {
      sg.undecodable++;
      return;
    }
    sg.order.push_back(id);
    sg.queue[(size_t) id].push_back(std::move(r));
  }
  // the segment's next message on `channel` (reading ahead past other channels' events if need be); false: none left
  bool pull(Seg &sg, int channel, Rec &out)
  {
    std::deque<Rec> &q = sg.queue[(size_t) channel];
    // (bounded: a live segment whose channel has stopped while its other channels go on would otherwise decode the whole rest of
    // its log into its queues in one tick -- the channel then simply has no message for this tick; SegmentStreamer keeps offsets
    // instead of decoded events and has the same bound)
    size_t ahead = 0;
    while (q.empty() && !sg.eof && ahead < readahead_cap) { read_one(sg); ahead++; }
    if (q.empty()) {
      if (!sg.eof) sg.capped++;
      return false;
    }
    out = std::move(q.front());
    q.pop_front();
    auto it = std::find(sg.order.begin(), sg.order.end(), channel);
    if (it != sg.order.begin()) sg.order_violations++;      // this segment's own log had something else first
    sg.order.erase(it);
    return true;
  }
  // smoothing: one batched IMU message's per-segment validity and message times (the handler gets the same mask)
  void keep_imu_tick(const std::vector<const Rec *> &col, const uint8_t *valid, int64_t utime)
  {
    if (terminal_ < 0) return;
    imu_tick_utime_.push_back(utime);
    imu_valid_.insert(imu_valid_.end(), valid, valid + B_);
    for (int s = 0; s < B_; s++) imu_utime_.push_back(col[(size_t) s] ? col[(size_t) s]->utime : 0);
  }
  // the runs of segments [first, first + count) are complete: keep their results (applies whatever the estimator holds back first)
  void finalize(int first, int count)
  {
    if (terminal_ >= 0) {   // smoothing: their posteriors at the end of their own logs, kept on the device (the newest step's "next")
      est_->flushPending();
      ending_.assign((size_t) B_, 0);
      std::fill_n(ending_.begin() + first, count, (uint8_t) 1);
      if (pb_slot_select(est_->ctx, terminal_, PB_SLOT_HEAD, ending_.data(), 1, PB_HOST) != PB_OK) {
        fprintf(stderr, "SegmentBatcher: %s\n", pb_last_error(est_->ctx));
        terminal_failed_ = true;   // (smooth() refuses: the terminal slot does not hold these segments' results)
      }
    }
    results_.finalize(est_, first, count, "SegmentBatcher");
  }
  // column s of a block's member at record offset `off` (`count` elements of T) <- the same member of a record
  template <class T>
  void put(uint8_t *blk, size_t off, size_t count, const uint8_t *rec, int s) const
  {
    T *dst = rows<T>(blk, off) + s;
    const T *src = segment_channels::member<T>(rec, off);
    for (size_t i = 0; i < count; i++) dst[i * (size_t) B_] = src[i];
  }
  template <class C>
  static std::function<bool(const pronto_wire::LogEvent &, Rec &, Stream &)> record_decoder(std::shared_ptr<C> ch, size_t bytes)
  {
    return [ch, bytes](const pronto_wire::LogEvent &ev, Rec &r, Stream &st) {
      r.bytes.resize(bytes);
      return ch->decode(ev.data.data(), ev.data.size(), st, r.bytes.data(), r.utime);
    };
  }
  template <class T>
  T *rows(uint8_t *blk, size_t off) const { return segment_channels::member<T>(blk, off, (size_t) B_); }   // a member's [count][B] rows in a block
  uint8_t *block(size_t rec_bytes)   // a zeroed page-locked [rec_bytes][B] block
  {
    uint8_t *p = pinned<uint8_t>(rec_bytes * (size_t) B_);
    std::fill_n(p, rec_bytes * (size_t) B_, (uint8_t) 0);
    return p;
  }
  template <class T>
  T *pinned(size_t n)
  {
    void *p = nullptr;
    if (pb_host_alloc(est_->ctx, sizeof(T) * (n ? n : 1), &p) != PB_OK) {
      fprintf(stderr, "SegmentBatcher: %s\n", pb_last_error(est_->ctx));
      exit(1);
    }
    pinned_.push_back(p);
    return (T *) p;
  }

  MavStateEstimator *est_;
  int B_;
  int64_t base_ = INT64_MIN;
  segment_channels::Results results_;
  std::vector<uint8_t> got_ = std::vector<uint8_t>((size_t) B_, 0);
  std::vector<std::unique_ptr<Seg>> segs_;
  std::map<std::string, Chan> chans_;
  std::vector<Chan *> chan_list_;
  std::vector<std::string> chan_names_;
  int first_alive_ = 0;
  std::vector<void *> pinned_, device_;
  int terminal_ = -1;                    // enableSmoothing: the estimator's checkpoint slot of the terminal posteriors
  bool terminal_failed_ = false;         // a copy into it failed
  std::vector<int64_t> imu_tick_utime_;  // per batched IMU message: its batch-level time ...
  std::vector<uint8_t> imu_valid_;       // ... [B] which segments had a message ...
  std::vector<int64_t> imu_utime_;       // ... [B] and their own message times
  std::vector<uint8_t> ending_;
};

}  // namespace MavStateEst
