/*
 * pronto_batch.h -- C ABI of the batched RBIS/RBIM EKF hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of openhumanoids/pronto: the propagate-and-correct loop
 * (RBISUpdateInterface::updateFilter of the IMU / indexed / indexed+orientation / reset updates, driven
 * by MavStateEstimator::addUpdate), batched over B independent filters.  Each entry point names the
 * reference interface it replaces (paths relative to the reference tree).  The reference has no FFI
 * today -- its boundary is C++; INTEGRATION.md shows the binding a maintainer would add,
 * and pronto_amd/csrc/mav_state_est_batch.hpp keeps the reference's class names on top of this ABI.
 *
 * Conventions
 *  - All functions return PB_OK (0) or an error code; they never throw and never exit().
 *    pb_last_error() gives the text of the last failure on that context.
 *  - The caller owns every buffer it passes; the context owns the device state.
 *  - One context is driven from one host thread at a time (the reference is single-threaded,
 *    lcm_front_end.cpp:223-229); distinct contexts (one per GPU) may be driven concurrently.
 *  - Batched arrays are SoA with the FILTER INDEX FASTEST: element (c, b) of an array [C][B] is at c*B + b.
 *  - `mem` says where the caller's buffers live: PB_HOST (copied into an internal device staging area on the
 *    context's stream, PCIe inclusive) or PB_DEVICE (HBM-resident; the kernels read them in place).
 *    PB_HOST_BROADCAST: host memory with ONE value per row, the same message for every filter (see enum pb_mem).
 *  - fp64 throughout.  State layout is RBIS's (rbis.hpp:22-30): vec = [omega(0-2) v_body(3-5) chi(6-8)
 *    pos(9-11) accel(12-14) | gyro_bias(15-17) accel_bias(18-20)], quat = (w,x,y,z), n_states = 15 keeps
 *    the first 15 (bias states and their covariance pinned to 0).
 *  - The covariance is stored symmetric-packed on the device; the reference does not symmetrise P
 *    (rbis.cpp:118,226) so results agree to rounding, not bit for bit (tolerances in tests/).
 */
#ifndef PRONTO_BATCH_H
#define PRONTO_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pb_ctx pb_ctx;

enum pb_status {
  PB_OK = 0,
  PB_ERR_ARG = 1,         /* bad argument (NULL, size, index out of range, unsupported m) */
  PB_ERR_HIP = 2,         /* a HIP runtime call failed; see pb_last_error */
  PB_ERR_NO_DEVICE = 3,   /* no gfx950 device / HIP extension unusable: there is NO CPU fallback */
  PB_ERR_STATE = 4        /* call order (e.g. step before reset, unknown snapshot slot) */
};

enum pb_mem {
  PB_HOST = 0,   /* caller's buffers are host memory, [rows][B] */
  PB_DEVICE = 1, /* caller's buffers are device memory, [rows][B] */
  /* host memory holding ONE value per row ([rows] doubles): the same message for every filter of the batch, the batch
   * differing in parameters / initial state only (the reference's own batch use: state-estimator/python/param_sweep.py:39-52
   * replays one log per parameter set).  Nothing of batch size crosses PCIe: the step kernels (pb_predict,
   * pb_step_legodo, pb_step_legodo_correct) and the handlers' index lists of pb_update_indexed(_orient) with a diagonal R
   * take the values as kernel arguments (no device block, no input traffic); any other block is expanded on the device.
   * Accepted by pb_predict, pb_update_indexed(_orient), pb_step_legodo(_correct), pb_legodo_update and pb_compose_delta;
   * mask must be NULL. */
  PB_HOST_BROADCAST = 2
};

/* how the measurement covariance R is passed to pb_update_indexed* */
enum pb_rkind {
  PB_R_DIAG_BROADCAST = 0, /* host double[m], same for every filter (handlers' cov_* members)       */
  PB_R_DIAG = 1,           /* [m][B]      per-filter diagonal (legodo certain/uncertain switch)       */
  PB_R_FULL = 2            /* [m*m][B]    per-filter full symmetric R, column-major (indexed_measurement_t) */
};

/* sensor ids, RBISUpdateInterface::sensor_enum (rbis_update_interface.hpp:10-12) */
enum pb_sensor {
  PB_SENSOR_INS = 0, PB_SENSOR_GPS, PB_SENSOR_VICON, PB_SENSOR_LASER, PB_SENSOR_LASER_GPF, PB_SENSOR_SCAN_MATCHER,
  PB_SENSOR_OPTICAL_FLOW, PB_SENSOR_RESET, PB_SENSOR_INVALID, PB_SENSOR_RGBD, PB_SENSOR_FOVIS, PB_SENSOR_LEGODO,
  PB_SENSOR_POSE_MEAS, PB_SENSOR_ALTIMETER, PB_SENSOR_AIRSPEED, PB_SENSOR_SIDESLIP, PB_SENSOR_INIT_MESSAGE,
  PB_SENSOR_VIEWER, PB_SENSOR_YAWLOCK
};

/* ---- lifetime ------------------------------------------------------------------------------------- */

/* Replaces MavStateEstimator::MavStateEstimator (mav_state_est.cpp:12-22) for B filters.
 * n_states in {15, 21}; device = HIP device ordinal; n_snapshots = history slots for pb_snapshot (>= 0). */
int pb_create(pb_ctx **out, int n_states, int batch, int device, int n_snapshots);
int pb_destroy(pb_ctx *ctx);
const char *pb_last_error(const pb_ctx *ctx); /* ctx may be NULL: last error of a failed pb_create */

/* A new context launches on its own non-blocking stream.  pb_set_stream switches to an existing hipStream_t, taken
 * literally: NULL is the null stream (torch's default stream) -- use the stream that PRODUCES the device buffers you
 * pass, otherwise nothing orders their producer kernels before these launches.  pb_use_own_stream switches back. */
int pb_set_stream(pb_ctx *ctx, void *hip_stream);
int pb_use_own_stream(pb_ctx *ctx);
/* eigen_utils constants that are not in the reference tree (g_vec magnitude, chiToQuat tolerance). */
int pb_set_constants(pb_ctx *ctx, double g, double chi_tol);
int pb_sync(pb_ctx *ctx);
/* name (as rocprofv3 prints it, without the pb:: prefix) of the kernel pb_step_legodo / pb_run_legodo launch for
 * this context: "k_step_coop<15,true,H>" (15 states, two waves per tile, up to 393 216 filters), "k_step<15,true,H>"
 * (15 states, one lane per filter, beyond that), "k_step_quad<true,H>" (21 states, four waves per tile) or
 * "k_step_coop<21,true,H>" (21 states with PRONTO_BATCH_QUAD21=0); H = 0/1/2 is the cache policy of the state round trip
 * the library picked from the state size (default / sc1 stores / non-temporal) */
const char *pb_hot_kernel(const pb_ctx *ctx);
/* filters per block of pb_run_legodo's cache-blocked order (0: the whole batch per launch; see pb_run_legodo) */
int pb_run_block(const pb_ctx *ctx);
int pb_batch(const pb_ctx *ctx);
int pb_n_states(const pb_ctx *ctx);

/* device memory helpers for hosts without torch (hipMalloc / hipMemcpy on the context's device) */
int pb_malloc(pb_ctx *ctx, uint64_t bytes, void **dev_ptr);
int pb_free(pb_ctx *ctx, void *dev_ptr);
int pb_memcpy_h2d(pb_ctx *ctx, void *dev_dst, const void *host_src, uint64_t bytes);
int pb_memcpy_d2h(pb_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
/* Page-locked host memory for PB_HOST inputs.  Any host memory works; from pinned buffers the staging copy is a DMA at
 * link rate, and either way it runs on a second stream into one of two staging buffers, so the copy of message k+1
 * overlaps the kernels of message k.  A PB_HOST call returns when its buffers have been copied (reusable at once). */
int pb_host_alloc(pb_ctx *ctx, uint64_t bytes, void **host_ptr);
int pb_host_free(pb_ctx *ctx, void *host_ptr);

/* ---- chunked uploads (bulk replays of recorded logs, segment_stream.hpp) ------------------------------------------------
 * The reference's LCMFrontEnd::run hands one message at a time to the handlers (lcm_front_end.cpp:223-229); a replay of N recorded
 * logs as one batch instead moves CHUNKS of pre-decoded messages ([slot][rows][B] blocks in page-locked memory) to HBM on the
 * context's copy stream while the kernels of the previous chunk run, and the handlers are then given PB_DEVICE messages.
 *   pb_fence_create / pb_fence_record   a marker on the main stream: "every kernel enqueued so far" (at most 16 per context)
 *   pb_fence_wait                       the host waits until the marked work has run
 *   pb_upload_async                     host (pb_host_alloc) -> device on the copy stream; it starts once fence `after_fence` has
 *                                       been reached (-1: at once) -- the fence recorded behind the last kernel that READ dev_dst
 *   pb_upload_join                      the main stream waits for every upload issued so far (call it before the first kernel
 *                                       that reads the uploaded block)
 *   pb_upload_sync                      the HOST waits for every upload issued so far (the page-locked source may be refilled) */
int pb_fence_create(pb_ctx *ctx, int *fence_out);
int pb_fence_record(pb_ctx *ctx, int fence);
int pb_fence_wait(pb_ctx *ctx, int fence);
int pb_upload_async(pb_ctx *ctx, void *dev_dst, const void *host_src, uint64_t bytes, int after_fence);
int pb_upload_join(pb_ctx *ctx);
int pb_upload_sync(pb_ctx *ctx);

/* ---- update objects (rbis_update_interface.hpp) ----------------------------------------------------- */

/* RBISResetUpdate::updateFilter (rbis_update_interface.cpp:23-28): posterior <- (state, cov), loglik <- 0.
 * vec [n][B], quat [4][B], cov [n*n][B] (full, column-major; the lower triangle is taken) -- or, with
 * broadcast != 0, vec [n], quat [4], cov [n*n] applied to every filter (host memory only). */
int pb_reset(pb_ctx *ctx, const double *vec, const double *quat, const double *cov, int broadcast, int mem);

/* The posterior of an update computed OUTSIDE the library becomes the head: posterior_state / posterior_covariance /
 * loglikelihood as an RBISUpdateInterface subclass fills them (rbis_update_interface.hpp:14-35; the estimator then reads them as
 * the next prior, mav_state_est.cpp:55-62).  This is the slow path behind the shim's RBISHostUpdate -- user code written against
 * the reference's updateFilter(const RBIS&, const RBIM&, double) runs on the host between a pb_get_head and this call.  Layout
 * as pb_reset (not broadcast); loglik [B] or NULL (= 0).  Honours pb_set_output_slot like every update.  PB_HOST or PB_DEVICE. */
int pb_set_head(pb_ctx *ctx, const double *vec, const double *quat, const double *cov, const double *loglik, int mem);

/* RBISIMUProcessStep::updateFilter (rbis_update_interface.cpp:30-52 -> rbis.cpp:37-122).
 * imu_block [7][B] = gyro xyz, accelerometer xyz (body frame, as InsHandler hands them over,
 * sensor_handlers.cpp:226-251), dt.  q = {q_gyro, q_accel, q_gyro_bias, q_accel_bias} (host). */
int pb_predict(pb_ctx *ctx, const double *imu_block, const double q[4], int mem);

/* RBISIndexedMeasurement::updateFilter (rbis_update_interface.cpp:54-95 -> rbis.cpp:160-178,124-143,219-227).
 * m in 1..6; idx host int[m] (state indices < n_states, distinct); z [m][B]; R per r_kind;
 * mask [B] uint8 or NULL: 0 = "handler returned NULL for this filter" (lcm_front_end.hpp:156) -> no update. */
int pb_update_indexed(pb_ctx *ctx, int m, const int *idx, const double *z, const double *R, int r_kind,
                      const uint8_t *mask, int mem);

/* RBISIndexedPlusOrientationMeasurement::updateFilter (rbis_update_interface.cpp:97-107 -> rbis.cpp:189-217).
 * quat_meas [4][B] (w,x,y,z).  z entries at chi indices (6..8) are ignored, as in the reference. */
int pb_update_indexed_orient(pb_ctx *ctx, int m, const int *idx, const double *z, const double *R, int r_kind,
                             const double *quat_meas, const uint8_t *mask, int mem);

#define PB_UPDATE_WIDE_MAX_ROWS 9
/* RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement::updateFilter for index lists of up to nine rows
 * (rbis.cpp:160-217; the GPF's all_states list {3..11}, rgbd_gpf_lib.cpp:86-91).  quat_meas == NULL: no orientation.
 * m in 1..9: up to six rows take exactly the path of pb_update_indexed / pb_update_indexed_orient (same kernel, same bits);
 * seven to nine run k_update_wide (one lane per filter, the measured columns in LDS); more is PB_ERR_ARG.  The two calls
 * above keep refusing m > 6.  Honoured as there: idx in range and distinct; all three pb_rkind encodings; mask [B];
 * PB_HOST, PB_DEVICE and PB_HOST_BROADCAST inputs (broadcast: mask must be NULL; a broadcast full R is expanded on the
 * device); pb_set_output_slot; a pending pb_set_pred_slot is refused; z entries at chi indices are ignored under an
 * orientation measurement; ONE log of the product of the pivots (rbis.cpp:142: NaN for a negative determinant).  A masked-off
 * filter keeps its state bit for bit. */
int pb_update_indexed_wide(pb_ctx *ctx, int m, const int *idx, const double *z, const double *R, int r_kind,
                           const double *quat_meas, const uint8_t *mask, int mem);

/* Fused hot step =RBISIMUProcessStep then RBISIndexedMeasurement(idx = velocityInds = {3,4,5}) as produced
 * by LegOdoCommon::createMeasurement in mode lin_rate (rbis_legodo_common.cpp:153-156): ONE launch and ONE
 * round trip of the state through HBM (BASELINE.json's "predict+update step").
 * lo_block [6][B] = z xyz, Rdiag xyz; mask as above. */
int pb_step_legodo(pb_ctx *ctx, const double *imu_block, const double *lo_block, const uint8_t *mask,
                   const double q[4], int mem);
/* The same step with the IMU block and the leg-odometry block (+ mask) living in DIFFERENT spaces, e.g. one robot's IMU
 * message for every filter (PB_HOST_BROADCAST) and a per-filter measurement that pb_legodo_update_after_predict left on
 * the device (PB_DEVICE).  At most one of the two may be PB_HOST. */
int pb_step_legodo_split(pb_ctx *ctx, const double *imu_block, int imu_mem, const double *lo_block, const uint8_t *mask,
                         int lo_mem, const double q[4]);

/* The same step with ONE MORE measurement behind it, still one launch and one round trip of the state: what the
 * reference does as a third updateFilter call when a correction message follows the IMU / leg-odometry pair.
 *   PB_CORR_POS_ORIENT  idx = {9,10,11,6,7,8}  FovisHandler position_orient (rbis_fovis_update.cpp:299-305)
 *   PB_CORR_POS_YAW     idx = {9,10,11,8}      ScanMatcherHandler position_yaw (sensor_handlers.cpp:709-722)
 * both RBISIndexedPlusOrientationMeasurement (rbis.cpp:189-217) with a diagonal R: z2 [m][B] (entries at chi indices are
 * ignored), R2 [m][B] (r_kind2 = PB_R_DIAG) or host double[m] (PB_R_DIAG_BROADCAST), quat_meas2 [4][B], mask2 [B] or NULL.
 * `mem` says where imu_block / lo_block / mask live, `mem2` where z2 / R2 / quat_meas2 / mask2 live (a FovisHandler
 * measurement is composed on the device, pb_compose_delta, while the IMU message comes from the host).
 * Results equal pb_step_legodo followed by pb_update_indexed_orient to rounding (tests/: <= 1e-12 relative). */
enum pb_corr { PB_CORR_POS_ORIENT = 0, PB_CORR_POS_YAW = 1 };
int pb_step_legodo_correct(pb_ctx *ctx, const double *imu_block, const double *lo_block, const uint8_t *mask,
                           const double q[4], int mem, int corr_kind, const double *z2, const double *R2, int r_kind2,
                           const double *quat_meas2, const uint8_t *mask2, int mem2);

/* n_steps consecutive fused steps from HBM-resident streams: imu_stream [n_steps][7][B],
 * lo_stream [n_steps][6][B], mask_stream [n_steps][B] or NULL (device pointers).  One launch per step (the
 * posterior is materialised in HBM after every message, as MavStateEstimator::addUpdate does,
 * mav_state_est.cpp:50-70).  If elapsed_ms != NULL the call brackets the launches with HIP events on the
 * context's stream, synchronises, and returns the device time.
 * Launch ORDER: for a state that fits the memory-side cache, step by step over the whole batch.  Beyond it (pb_create: more than
 * 256 MB of state and a batch of whole tiles; pb_run_block() > 0) the call runs filter range OUTER, time INNER: a block of
 * pb_run_block() filters takes all n_steps steps -- its posteriors stay cache-resident from step to step -- before the next block
 * starts.  The filters are independent, so the results are those of the step-by-step order: bit for bit when the same step kernel
 * runs (PRONTO_BATCH_COOP15 forced, or any batch up to 393 216 filters), to rounding where the blocks run the two-wave 15-state
 * kernel that their size wants and the whole batch would run the one-lane kernel.  Same accounting as ever: one launch per step
 * and block, every posterior loaded and stored once per step.  PRONTO_BATCH_BLOCKED=0 keeps the step-by-step order. */
int pb_run_legodo(pb_ctx *ctx, int n_steps, const double *imu_stream, const double *lo_stream,
                  const uint8_t *mask_stream, const double q[4], float *elapsed_ms);

/* Time-fused replay of the same streams: steps_per_launch consecutive steps per kernel launch with the state and
 * covariance resident in registers; the posterior is written to HBM once per launch instead of once per message.  Same
 * arithmetic as pb_run_legodo, NOT the plugin semantics (no per-message posterior): meant for parameter sweeps and
 * likelihood evaluation over log segments (state-estimator/python/param_sweep.py:39-52).  15 states: k_replay_coop (two
 * waves per tile), 21 states: k_replay_quad (four).  Accounting differs from the T = 1 path (104 + 2240/T bytes per
 * 15-state filter-step, 104 + 4112/T for 21 states): see DESIGN.md section 6. */
int pb_replay_legodo_fused(pb_ctx *ctx, int n_steps, int steps_per_launch, const double *imu_stream,
                           const double *lo_stream, const uint8_t *mask_stream, const double q[4], float *elapsed_ms);

/* The same replay as a forward pass that KEEPS EVERY POSTERIOR -- what the reference's history does by value
 * (mav_state_est.cpp:50-70) and what EKFSmoothBackwardsPass reads (:98-189): the posterior of step t is also written into
 * checkpoint slot first_slot + t (pb_history_reserve; first_slot + n_steps <= slots), while the state stays in registers.
 * Per step one slot is written and nothing is read back (the per-message path with pb_set_output_slot reads the previous
 * slot and writes the next one).  Slots are bit-identical to pb_replay_legodo_fused run ONE step per launch, and equal to
 * rounding (1e-12 relative in the tests) to what pb_set_output_slot + pb_step_legodo leave -- another kernel, other FMA
 * contractions: do not mix the two paths under a bit-exact replay checksum.  The head
 * afterwards is the context's own array (= the last slot's content).  Accounting: (S_x + S_P + 8) + 104 + 2 (S_x + S_P + 8) / T
 * bytes per filter-step -- its own, never the headline metric. */
int pb_replay_legodo_checkpointed(pb_ctx *ctx, int n_steps, int steps_per_launch, const double *imu_stream,
                                  const double *lo_stream, const uint8_t *mask_stream, const double q[4], int first_slot,
                                  float *elapsed_ms);

/* ---- history look-up used by FovisHandler (rbis_fovis_update.cpp:184-223) ------------------------------ */

/* remember the head posterior's (position, quat) in `slot` (the reference finds it again by
 * history.updateMap.lower_bound(prev_timestamp)) */
int pb_snapshot(pb_ctx *ctx, int slot);
/* the same from a saved posterior (pb_history_reserve checkpoint) instead of the head: what FovisHandler does when the
 * keyframe changes -- history.updateMap.lower_bound(prev_timestamp)->posterior_state (rbis_fovis_update.cpp:184-207) */
int pb_snapshot_from_slot(pb_ctx *ctx, int slot, int checkpoint_slot);
/* T1 = T0(slot) * (t, q): z_out [3][B] = T1.translation, quat_out [4][B] = T1.rotation (device buffers) */
int pb_compose_delta(pb_ctx *ctx, int slot, const double *t, const double *q, double *z_out, double *quat_out,
                     int mem);

/* ---- noise identification / parameter sweeps (state-estimator/src/noise_id/noise_id.cpp:9-65) ------------------ */

/* Per-filter process noise: q_block [4][B] (device memory) = q_gyro, q_accel, q_gyro_bias, q_accel_bias of every
 * filter, used instead of the scalar q of the call by EVERY following call that takes a process step; NULL switches back.  The
 * block is read in place at each launch (keep it alive and unchanged while calls are in flight).  The calls that honour it:
 *   pb_predict, pb_step_legodo, pb_step_legodo_split, pb_step_legodo_correct -- with or without pb_set_output_slot /
 *     pb_set_pred_slot (the predicted slot holds the per-filter process step) and under pb_set_imu_valid (what is put back for an
 *     idle filter is measured against ITS q);
 *   pb_run_legodo in both launch orders (the cache-blocked order hands every block of filters its own columns of q_block);
 *   pb_replay_legodo_fused, pb_replay_legodo_checkpointed;
 *   pb_step_legodo_feet, pb_step_legodo_joints, alone or together with pb_legodo_set_param_block;
 *   pb_smooth_log, pb_smooth_log_fused, pb_smooth_log_corrected (the forward and the recompute pass).
 * 15 states have no bias states: rows 2 and 3 are never read into the arithmetic there.  tests/test_process_noise_block.py holds
 * each of these against the oracle run with every filter's own q.  This is what lets ONE batch carry the windows x candidate-noise
 * grid of a noise-ID run (sampleProcessForward, noise_id.cpp:9-42: by linearity rolled_cov - start_window_cov is the predict chain
 * from P = 0) or a process-noise sweep over one log (examples/param_sweep.c). */
int pb_set_process_noise_block(pb_ctx *ctx, const double *q_block_dev);
/* Window likelihood pieces (noise_id.cpp:37-38,44-65): e = head (-) truth with chi = Log(truth.quat^-1 * quat); over
 * the m <= 9 active indices: out3 [3][B] = log det P_aa, e_a^T P_aa^-1 e_a, -0.5*(m log 2pi + logdet + maha).
 * truth_vec [n][B], truth_quat [4][B]; err_out [n][B] or NULL. */
int pb_window_nll(pb_ctx *ctx, int m, const int *idx, const double *truth_vec, const double *truth_quat, double *out3,
                  double *err_out, int mem);

/* ---- leg kinematic odometry: the producer of the leg-odometry increment LegOdoHandler turns into a measurement ----
 * Replaces, per filter, leg_estimate::updateOdometry (motion_estimate/src/leg_estimate/leg_estimate.cpp:395-556: forward
 * kinematics :430-447, 30 ms reset, primary-foot selection through FootContactAlt::DetectFootTransition or -- contact mode
 * "standing" -- FootContact::DetectFootTransition, pelvis pose slaved to the FILTER's own orientation, :219-297) and
 * foot_contact_classify::update (foot_contact_classify.cpp:57-125: status -1 / 0 / 1).  Inputs are either the two
 * body-to-foot transforms (pb_legodo_update*: feet [14][B] = body-to-left-foot (t3, q4 = w,x,y,z), body-to-right-foot
 * (t3, q4); forces [2][B] = left, right |vertical foot force|, doubles) or the joint state itself (pb_legodo_update_joints,
 * after pb_legodo_set_chain).  `mem` as everywhere (PB_HOST_BROADCAST: one robot's message for a whole parameter sweep).
 * Outputs are DEVICE arrays, any may be NULL: delta_out [7][B] (pelvis increment t3, q4),
 * status_out [B], and -- LegOdoCommon::createMeasurement in mode lin_rate (rbis_legodo_common.cpp:99-169) -- lo_block_out
 * [6][B] + mask_out [B] in exactly the form pb_step_legodo / pb_update_indexed take with PB_DEVICE.
 * The thresholds are rounded to float like the reference's (leg_estimate.cpp:103-104); delays < 2e9 us. */
int pb_legodo_init(pb_ctx *ctx, double schmitt_low_threshold, double schmitt_high_threshold, int64_t schmitt_low_delay_us,
                   int64_t schmitt_high_delay_us, int filter_contact_events);
int pb_legodo_update(pb_ctx *ctx, int64_t utime, const double *feet, const double *forces, int mem, int zero_delta,
                     double r_vxyz, double r_vxyz_uncertain, double *delta_out, double *status_out, double *lo_block_out,
                     uint8_t *mask_out);
/* The same odometry, slaved to the orientation the filter WILL have after pb_predict(imu_block) -- computed from the head
 * state on the device, covariance untouched -- so that the caller can then run that IMU step and the leg-odometry update this
 * call produced as ONE fused kernel (pb_step_legodo_split with lo_block_out / mask_out as PB_DEVICE blocks) instead of
 * pb_predict, pb_legodo_update, pb_update_indexed: two state round trips become one.  Results equal that three-call sequence
 * to rounding.  imu_block: [7][B] (PB_DEVICE / PB_HOST) or [7] (PB_HOST_BROADCAST); not both it and the foot blocks PB_HOST. */
int pb_legodo_update_after_predict(pb_ctx *ctx, const double *imu_block, int imu_mem, int64_t utime, const double *feet,
                                   const double *forces, int mem, int zero_delta, double r_vxyz, double r_vxyz_uncertain,
                                   double *delta_out, double *status_out, double *lo_block_out, uint8_t *mask_out);
/* Contact mode (leg_estimate.cpp:113-121): standing != 0 = state_estimator.legodo.init_contact_mode "standing", the
 * conservative FootContact classifier (foot_contact/FootContact.cpp:29-54; total_force and standing_schmitt_level are floats
 * there and here); use_controller_input != 0 lets the controller's contact counts overrule FootContactAlt's standing foot
 * (leg_estimate.cpp:365-387).  Call after pb_legodo_init, which puts EVERYTHING back to the constructor's defaults: FootContactAlt,
 * no controller input, controller contact counts -1, no world constraint, all per-robot state reset. */
int pb_legodo_set_contact_mode(pb_ctx *ctx, int standing, double total_force, double standing_schmitt_level,
                               int use_controller_input);
/* Independent log segments (one recorded robot per filter; the reference's se-batch-process.sh runs such logs one after the
 * other): every filter's message carries its OWN time stamp, and a filter whose segment has ended has none.  For the NEXT
 * odometry / pair call only: utimes [B] (int64, may be NULL = the call's scalar utime for every filter) is what
 * leg_estimate::updateOdometry takes as `utime` per filter (elapsed time of the increment, the 30 ms reset, the Schmitt-trigger
 * clocks, foot_contact_classify's black-out windows); valid [B] (uint8, may be NULL = all) marks the filters that HAVE a message --
 * the others keep their odometry state and get no measurement (mask 0).  mem: PB_HOST (copied before the call returns) or
 * PB_DEVICE (read IN PLACE by the consuming launch: the arrays stay the caller's until that launch has run).  The arrays are
 * taken by the next pb_legodo_update* / pb_step_legodo_joints / _feet call whatever its outcome -- a call that fails its argument
 * checks has still consumed them.  (The joint Kalman filter of
 * pb_joint_filter keeps one clock per context: with per-filter times use the low-pass filter or none.) */
int pb_legodo_set_message_times(pb_ctx *ctx, const int64_t *utimes, const uint8_t *valid, int mem);
/* Which of LegOdoCommon's measurements (state_estimator.legodo.mode, rbis_legodo_common.cpp:5-23,110-169) the odometry calls
 * pb_legodo_update / _after_predict / _joints write into lo_block_out / mask_out -- formed on the device, where the increment
 * is, so that no batch-sized array crosses PCIe to form it (the reference forms it on the host right behind updateOdometry):
 *   0  lin_rate (default)  lo_block_out [6][B]  = z (v), Rdiag;                  mask_out [B]     idx {3,4,5}
 *   1  lin_rot_rate        lo_block_out [12][B] = z (v, rpy rate) [6], Rdiag [6]; mask_out [B]     idx {3,4,5,0,1,2}
 *   2  pos_and_lin_rate    lo_block_out [12][B] = z (position, v) [6], Rdiag [6]; mask_out [2][B]  idx {9,10,11,3,4,5}
 *      mask_out[0][b] = status valid AND position valid: the six-row update; mask_out[1][b] = status valid AND position NOT valid:
 *      the reference's per-message fall-back to lin_rate (:118-122), a three-row update on rows 3..5 (z) and 9..11 (Rdiag) of
 *      the same block with idx {3,4,5}.  (The position is leg_estimate's world constraint, which this mode switches on.)
 * r_xyz, r_vang, r_vang_uncertain: state_estimator.legodo.r_xyz / r_vang / r_vang_uncertain (r_vxyz and r_vxyz_uncertain stay
 * arguments of the odometry calls).  The pair calls pb_step_legodo_joints / _feet form AND APPLY the same measurement (their
 * lo_block_out / mask_out have the shapes above).  pb_legodo_init puts the mode back to 0. */
int pb_legodo_set_measurement_mode(pb_ctx *ctx, int mode, double r_xyz, double r_vang, double r_vang_uncertain);
/* Parameter sweeps over the measurement side of the leg odometry (state-estimator/python/param_sweep.py:39-52, one process per
 * `-O key=value` there): the eleven state_estimator.legodo.* scalars PER FILTER.  block [PB_LEGPAR_ROWS][B], rows in the .cfg's units:
 *   PB_LEGPAR_R_VXYZ, _R_VXYZ_UNCERTAIN                       the r_vxyz / r_vxyz_uncertain arguments of every odometry / pair call
 *   PB_LEGPAR_R_VANG, _R_VANG_UNCERTAIN, _R_XYZ               pb_legodo_set_measurement_mode's
 *   PB_LEGPAR_SCHMITT_LOW, _HIGH, _LOW_DELAY, _HIGH_DELAY     pb_legodo_init's (delays in us, whole numbers)
 *   PB_LEGPAR_TOTAL_FORCE, _STANDING_SCHMITT_LEVEL            pb_legodo_set_contact_mode's
 * The noises are standard deviations, squared where they are used; thresholds, total_force and the level pass through `float` as in
 * the scalar setters: a block that holds one value per row gives the bits of the scalar calls.  While a block is set its rows replace
 * those scalars in every pb_legodo_update* and pb_step_legodo_joints / _feet call, and the calls' r_vxyz / r_vxyz_uncertain arguments
 * are ignored; the flags and modes (filter_contact_events, standing, use_controller_input, the measurement mode) stay per context.
 * mem = PB_HOST or PB_DEVICE (PB_HOST_BROADCAST: PB_ERR_ARG); either way the block is copied into memory the context owns before the
 * call returns.  A PB_HOST block is checked per filter -- noises finite and >= 0, high >= low threshold, delays whole numbers in
 * [0, 2e9] -- and the first offending filter and row are named in pb_last_error (PB_ERR_ARG; the block set before, or none, stays in
 * force).  A PB_DEVICE BLOCK IS COPIED UNCHECKED: the same rules are the caller's to keep.  block = NULL switches back to the scalars;
 * so does pb_legodo_init.  PB_ERR_STATE before pb_legodo_init. */
enum { PB_LEGPAR_R_VXYZ = 0, PB_LEGPAR_R_VXYZ_UNCERTAIN, PB_LEGPAR_R_VANG, PB_LEGPAR_R_VANG_UNCERTAIN, PB_LEGPAR_R_XYZ,
       PB_LEGPAR_SCHMITT_LOW, PB_LEGPAR_SCHMITT_HIGH, PB_LEGPAR_SCHMITT_LOW_DELAY, PB_LEGPAR_SCHMITT_HIGH_DELAY,
       PB_LEGPAR_TOTAL_FORCE, PB_LEGPAR_STANDING_SCHMITT_LEVEL, PB_LEGPAR_ROWS };
int pb_legodo_set_param_block(pb_ctx *ctx, const double *block /* [PB_LEGPAR_ROWS][B] */, int mem);
/* LegOdoHandler's "ignore the calculated velocity at launch" (state_estimator.legodo.zero_initial_velocity,
 * rbis_legodo_update.cpp:58,264-268), counted PER FILTER on the device: the counter is decremented by every message whose
 * status is valid for that filter (the reference returns NULL before the decrement otherwise, :243-255) and while it stays
 * above zero the increment (and the position) handed on is the identity.  Independent of the per-call zero_delta flag.
 * ticks <= 65535 (the counter is a 16-bit field of the per-robot flag word), else PB_ERR_ARG. */
int pb_legodo_set_zero_initial_velocity(pb_ctx *ctx, int ticks);
/* The last CONTROLLER_FOOT_CONTACT message (LegOdoHandler::controllerInputHandler, rbis_legodo_update.cpp:190-193):
 * n_contacts = {num_left_foot_contacts, num_right_foot_contacts} for every filter (PB_HOST_BROADCAST) or [2][B]
 * (PB_HOST / PB_DEVICE); kept until the next call; before the first call both are -1 (rbis_legodo_update.cpp:100-101). */
int pb_legodo_set_control_contacts(pb_ctx *ctx, const int32_t *n_contacts, int mem);
/* Forward kinematics table: what kdl_parser + KDL::TreeFkSolverPosFull_recursive make of the URDF for the two standing links
 * (leg_estimate.cpp:68-73,430-447; state_estimator.legodo.{left,right}_standing_link).  KDL and the URDF are not part of the
 * reference tree, so the caller supplies, for the joints from the root link down to each standing link (left chain first,
 * n_left + n_right entries): joint_type (0 fixed, 1 revolute / continuous, 2 prismatic), joint_row (row of the joint-position
 * block that holds the joint, i.e. its index in joint_state_t.joint_name), origin_xyz_rpy [.][6] (the URDF <origin>),
 * axis [.][3] (the URDF <axis>, normalised here like KDL::Joint does), adjustment_gain [.] or NULL
 * (state_estimator.legodo.adjustment_gain of that joint, EstimateTools::TorqueAdjustment: 0, inf or nan = none).
 * body_to_foot = prod_j [R(rpy_j), xyz_j] * Rot(axis_j, position_j).  At most 8 joints per leg. */
int pb_legodo_set_chain(pb_ctx *ctx, int n_left, int n_right, const int *joint_type, const int *joint_row,
                        const double *origin_xyz_rpy, const double *axis, const float *adjustment_gain);
/* leg_estimate::updateOdometry from a joint state: joint_position [n_rows][B] floats (bot_core::joint_state_t carries
 * floats), joint_effort [n_rows][B] or NULL (torque adjustment off, rbis_legodo_update.cpp:236-238), forces [2][B] floats
 * (FootSensing::force_z).  PB_HOST_BROADCAST: [n_rows] / [2] values of ONE robot.  imu_block != NULL: slaved to the
 * orientation after that IMU step, as pb_legodo_update_after_predict.  position_out [3][B] + position_status_out [B]
 * (DEVICE, may be NULL): the pelvis position leg_estimate derives from the foot it last put down
 * (getLegOdometryWorldConstraint, leg_estimate.cpp:299-318,461-492: world_to_body_constraint_ and its _init_ flag), which
 * LegOdoCommon's mode pos_and_lin_rate measures; it is tracked from the first call that passes position_out.
 * Everything else as pb_legodo_update. */
int pb_legodo_update_joints(pb_ctx *ctx, const double *imu_block, int imu_mem, int64_t utime, int n_rows,
                            const float *joint_position, const float *joint_effort, const float *forces, int mem, int zero_delta,
                            double r_vxyz, double r_vxyz_uncertain, double *delta_out, double *status_out, double *lo_block_out,
                            uint8_t *mask_out, double *position_out, uint8_t *position_status_out);
/* ONE call per IMU + joint-state (or foot-state) message pair -- RBISIMUProcessStep::updateFilter, leg_estimate::updateOdometry
 * slaved to the head AFTER that step, LegOdoCommon::createMeasurement (the mode of pb_legodo_set_measurement_mode; default
 * lin_rate) and RBISIndexedMeasurement::updateFilter (rbis_update_interface.cpp:30-95, rbis_legodo_update.cpp:206-280) -- and ONE
 * kernel and one round trip of the filter state: k_step_leg for 15 states up to 393 216 filters, k_step_quad_leg for 21; other
 * contexts run pb_legodo_update_joints(imu_block, ...) followed by pb_step_legodo_split (lin_rate) or pb_predict and
 * pb_update_indexed (the six-row modes) internally.  Results equal that sequence (tests: bit-identical statuses, posterior to
 * rounding).  The six-row modes are applied as their two 3-row blocks with ONE summed correction -- R is diagonal, so that IS the
 * six-row update (equal to rounding, not bit for bit: the 6 x 6 S is never factored); mode 2's per-filter fall-back to lin_rate
 * is the velocity block alone.  imu_block / imu_mem and q as pb_step_legodo; the leg inputs as pb_legodo_update_joints /
 * pb_legodo_update; not both groups PB_HOST.  lo_block_out + mask_out (DEVICE, or both NULL; [6][B] + [B], six-row modes [12][B] +
 * [B] / [2][B]): the measurement that was applied, for a caller that may have to re-apply this update later (history replay) --
 * the odometry itself must not run twice. */
int pb_step_legodo_joints(pb_ctx *ctx, const double *imu_block, int imu_mem, const double q[4], int64_t utime, int n_rows,
                          const float *joint_position, const float *joint_effort, const float *forces, int mem, double r_vxyz,
                          double r_vxyz_uncertain, double *lo_block_out, uint8_t *mask_out);
int pb_step_legodo_feet(pb_ctx *ctx, const double *imu_block, int imu_mem, const double q[4], int64_t utime, const double *feet,
                        const double *forces, int mem, double r_vxyz, double r_vxyz_uncertain, double *lo_block_out,
                        uint8_t *mask_out);
/* The joint-position filters in front of the kinematics -- step 0 of leg_estimate::updateOdometry (leg_estimate.cpp:411-428,
 * state_estimator.legodo.filter_joint_positions): mode 1 = LowPassFilter (estimate_tools filter_tools/Filter.cpp:4-65: 14-tap
 * FIR, the first sample fills the window), mode 2 = SimpleKalmanFilter (kalman_filter_tools/simple_kalman_filter.cpp:11-50;
 * the three noise values are its constructor arguments -- leg_estimate.cpp:56 passes (joint_process_noise,
 * joint_observation_noise) and leaves the third at 5e-4 -- kept as floats like its members).  One filter per robot and joint
 * ROW THE KINEMATIC CHAINS READ (pb_legodo_set_chain first; setting another chain invalidates the filters) with row < 28
 * (NUM_FILT_JOINTS, leg_estimate.hpp:59); pb_joint_filter_init starts every filter over.
 * pb_joint_filter: one joint_state_t message per robot, [n_rows][B] floats (PB_HOST / PB_DEVICE; joint_position_out is a
 * DEVICE array [n_rows][B] to be handed to pb_legodo_update_joints / pb_step_legodo_joints as PB_DEVICE) or ONE robot's
 * [n_rows] values (PB_HOST_BROADCAST; joint_position_out is a HOST array [n_rows] to be passed on as PB_HOST_BROADCAST).
 * joint_velocity: read by the Kalman filter's first sample only (may be NULL for the low-pass).  joint_effort != NULL: the
 * handler's torque adjustment (rbis_legodo_update.cpp:231-241, gains of pb_legodo_set_chain) is applied BEFORE the filters
 * as in the reference -- pass joint_effort = NULL to the kinematics afterwards.  Filtered positions are rounded to float
 * like the reference's std::vector<float> (leg_estimate.hpp:91-93); rows no filter owns are copied. */
int pb_joint_filter_init(pb_ctx *ctx, int mode, double process_noise_pos, double process_noise_vel, double observation_noise);
int pb_joint_filter(pb_ctx *ctx, int64_t utime, int n_rows, const float *joint_position, const float *joint_velocity,
                    const float *joint_effort, int mem, float *joint_position_out);
/* forward kinematics alone (diagnostics, tests): feet_out [14][B] DEVICE array in pb_legodo_update's layout */
int pb_legodo_fk(pb_ctx *ctx, int n_rows, const float *joint_position, const float *joint_effort, int mem, double *feet_out);
/* one filter's odometry state, for diagnostics and tests: odom_to_body (t3, q4); info = primary_foot (0 left, 1 right),
 * leg_odo_init, walking-phase mode (foot_contact_classify.hpp:34-44), transitions the classifier did not know */
int pb_legodo_get(pb_ctx *ctx, int filter, double odom_to_body[7], int64_t info[4]);

/* ---- yaw lock (YawLockHandler, motion_estimate/src/quick_lock/rbis_yawlock_update.cpp; YawLock::getCorrection,
 * yawlock.cpp:78-205) ------------------------------------------------------------------------------------------------
 * While the robot stands, the pose the two standing links had when it came to stand and the leg kinematics now give a
 * drift-free pelvis orientation (the yaw row of an indexed + orientation measurement), and the body-frame gyro z is a
 * measurement of the gyro bias z.  The handler is a small state machine PER FILTER -- it reads the filter's own head pose -- kept in
 * a context-owned array: the two captured world-to-foot poses, the captured left-to-right rotation, utime_disable_until, the
 * counter, lock_init, and the number of slips detected (the reference publishes YAW_SLIP_DETECTED instead).
 * The kinematic chain is the one of pb_legodo_set_chain (PB_ERR_STATE without one); joint positions are the RAW message values:
 * no joint filter, no torque adjustment (rbis_yawlock_update.cpp:188).
 *
 * pb_yawlock_init: mode 0 yawbias (idx {17}), 1 yaw (idx {8}), 2 yawbias_yaw (idx {17, 8}); modes 0 and 2 need the 21-state
 * filter (PB_ERR_ARG on 15 states).  correction_period >= 1.  yaw_slip_disable_period_s: the reference reads it from the key
 * state_estimator.yawlock.yaw_slip_threshold_degrees (rbis_yawlock_update.cpp:19) -- pass what the caller's configuration gives.
 * r_yaw_bias_deg / r_yaw_deg: R = (r pi/180)^2.  Every filter's state goes back to the constructor's: counter 0, no lock,
 * disable_until 0; standing false and gyro z 0 for every filter. */
int pb_yawlock_init(pb_ctx *ctx, int mode, int correction_period, int yaw_slip_detect, double yaw_slip_threshold_degrees,
                    double yaw_slip_disable_period_s, double r_yaw_bias_deg, double r_yaw_deg);
/* What the status handlers (controllerStatusHandler / robotBehaviorHandler) and insHandler keep, until the next call: ONE value
 * for every filter (PB_HOST_BROADCAST) or [B] values (PB_HOST / PB_DEVICE; copied before the call returns). */
int pb_yawlock_set_standing(pb_ctx *ctx, const uint8_t *standing, int mem);
int pb_yawlock_set_gyro(pb_ctx *ctx, const double *body_gyro_z, int mem);
/* YawLockHandler::processMessage for every filter, FORM only (diagnostics; a caller that applies the update later): runs the
 * state machine and writes (DEVICE arrays, each may be NULL)
 *   z_out [2][B]     row 0 = the bias measurement (gyro z while standing, else the head's own gyro bias z), row 1 = 0
 *   quat_out [4][B]  the orientation measurement (w x y z; identity where there is none)
 *   mask_out [2][B]  row 0: apply the mode's row set with the orientation (pb_update_indexed_orient with idx {8} / {17, 8},
 *                    R = {r_yaw^2} / {r_yaw_bias^2, r_yaw^2}); row 1: apply the bias row alone (pb_update_indexed, idx {17}).
 *                    Neither = the handler returned NULL for this filter.
 * joint_position: [n_rows][B] floats (PB_HOST / PB_DEVICE) or ONE robot's [n_rows] values (PB_HOST_BROADCAST).
 * utimes / valid: DEVICE arrays [B] or NULL (batches of independent log segments): the message time per filter instead of
 * `utime`; valid == 0 = no message for this filter, which keeps its state, its counter included.  The filter state is not touched. */
int pb_yawlock_update_joints(pb_ctx *ctx, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows,
                             const float *joint_position, int mem, double *z_out, double *quat_out, uint8_t *mask_out);
/* The same, formed AND APPLIED in one kernel (k_step_yawlock): a filter without an update leaves after the small read without
 * touching its covariance; one with an update makes one round trip of its state.  Equal to pb_yawlock_update_joints followed by
 * pb_update_indexed_orient / pb_update_indexed with the two masks, to rounding.  Honours pb_set_output_slot; writes no predicted
 * posterior (a pending pb_set_pred_slot is refused and forgotten).  The optional outputs are the measurement that was applied,
 * for a caller that may have to re-apply it later (history replay) -- the state machine itself must not run twice. */
int pb_step_yawlock_joints(pb_ctx *ctx, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows,
                           const float *joint_position, int mem, double *z_out, double *quat_out, uint8_t *mask_out);
/* one filter's yaw-lock state, for diagnostics and tests: poses = world_to_l_foot_original, world_to_r_foot_original (t3, q4
 * each); info = counter, lock_init, utime_disable_until, last outcome (low 8 bits: 0 no message, 1 not a correction tick, 2 not
 * standing, 3 held off after a slip, 4 captured, 5 slip detected, 6 correction, 7 mode yawbias; the rest: slips so far << 8) */
int pb_yawlock_get(pb_ctx *ctx, int filter, double poses[14], int64_t info[4]);

/* ---- IMU front end of the Atlas path (InsHandler::doFilter, sensor_handlers.cpp:29-42,154-162) ---------------- */

/* Three cascaded 2nd-order IIR notches (iir_notch.cpp:3-61) at notch_freq * 2^i, i = 0..2, per accelerometer axis and
 * per filter.  pb_imu_notch_init allocates/zeroes the per-filter filter state and fixes the coefficients
 * (state_estimator.ins.atlas_filter_freq, fs = 1000 in the reference). */
int pb_imu_notch_init(pb_ctx *ctx, double notch_freq, double fs);
/* Filters n_packets consecutive NEW packets (oldest first) accel_packets [n_packets][3][B]; accel_out [3][B] receives
 * the newest filtered sample (what processMessageAtlas feeds to the process step, sensor_handlers.cpp:191-196).
 * accel_out must be device memory when mem == PB_DEVICE, host memory when PB_HOST. */
int pb_imu_notch(pb_ctx *ctx, int n_packets, const double *accel_packets, double *accel_out, int mem);
/* The same with a PER-FILTER packet count -- independent log segments: every filter has its own KVH stream and its own
 * IMUStream de-duplication (imu_stream.cpp:62-98), so a batched message carries a different number of NEW packets per filter.
 * counts [B] (int32): filter b runs its first min(counts[b], max_packets) packets of accel_packets [max_packets][3][B] (oldest
 * first) through its cascade; a filter with no new packet keeps its filter state and its accel_out entries are not written
 * (PB_HOST: they come back as 0) -- the reference returns NULL for such a message (sensor_handlers.cpp:181-187). */
int pb_imu_notch_counts(pb_ctx *ctx, int max_packets, const int32_t *counts, const double *accel_packets, double *accel_out, int mem);

/* InsHandler's per-message arithmetic for B robots at once, on the device: one robot's IMU sample -> the [7][B] block that
 * pb_predict / pb_step_legodo* take (gyro xyz | accelerometer xyz | dt, body frame), written to imu_block_out (DEVICE memory).
 *   Microstrain (InsHandler::processMessage, sensor_handlers.cpp:96-131): gyro [3][B] and accel [3][B] rotated by rot_quat
 *     (bot_quat_rotate_to), dt = dt_default.  raw_dt = NULL, trans_vec = NULL, dt_from_utimes = 0.
 *   Atlas KVH (processMessageAtlas, :199-252): gyro holds delta_rotation and is divided by raw_dt [B] (:207-210); accel goes through
 *     the whole ins_to_body transform (rotation + trans_vec, bot_trans_apply_vec :227); dt_from_utimes = 1: dt = (utime - this
 *     filter's previous utime) * 1E-6, dt_default on its first message (:239-249).  utimes [B] = every robot's own message time,
 *     or NULL = `utime` for all.
 *   valid [B] (or NULL = all): 0 = this filter has NO message (its log segment has ended, or its KVH batch carried no new packet:
 *     the reference's handler returns NULL) -- its block entry is its own last sample with dt = 0; its previous-utime is not
 *     advanced.  valid_out (DEVICE, [B], or NULL) receives the mask: hand it to pb_set_imu_valid in front of the call that takes the
 *     step, which makes that step a no-op for these filters.
 * mem (of the input arrays): PB_HOST or PB_DEVICE.  pb_ins_body_reset forgets the last samples / previous utimes. */
int pb_ins_body_block(pb_ctx *ctx, const double *gyro, const double *accel, const double *raw_dt, const int64_t *utimes, int64_t utime,
                      const uint8_t *valid, const double rot_quat[4], const double trans_vec[3], double dt_default, int dt_from_utimes,
                      int mem, double *imu_block_out, uint8_t *valid_out);
int pb_ins_body_reset(pb_ctx *ctx);
/* Filters WITHOUT an IMU message in the next IMU step (independent log segments: the reference's handler returned NULL for them, so
 * its estimator did nothing at all).  valid_dev [B] (DEVICE; 0 = no message) applies to the NEXT call that takes an IMU step
 * (pb_predict, pb_step_legodo, _split, _correct, pb_step_legodo_joints / _feet) and is consumed by it whatever its outcome.  A
 * step with dt = 0 already leaves pose, velocity, biases and covariance alone whatever the sample; with the mask the library
 * replaces, right in front of the step kernel, the sample of such a filter by the one that reproduces its angular-velocity and
 * acceleration entries too (omega + gyro bias, a + accel bias of the prior), and sets its dt to 0: the step is a no-op for it --
 * exactly for 15 states, to the last bit of those sums for 21 -- and a measurement update in the same kernel sees the state the
 * reference's would.  One thing a process step does whatever dt: it overwrites the angular-velocity and the acceleration diagonal
 * block of the covariance with q_gyro I and q_accel I (rbis.cpp:120-121); behind the step kernel the library puts the prior's blocks
 * back for these filters (bit for bit; where a correction in the same call has downdated them, with that downdate kept).
 * The step kernels themselves know nothing of it.  The array must stay valid until the step has run.
 * The mask applies wherever that call's IMU sample lives: a PB_HOST_BROADCAST sample (one for every filter, otherwise passed as
 * kernel arguments) is covered too -- under a mask it is expanded on the device into the prepared block the step reads. */
int pb_set_imu_valid(pb_ctx *ctx, const uint8_t *valid_dev);

/* ---- posterior checkpoints for roll-forward replay (mav_state_est.cpp:28-80, update_history.cpp) ------------ */

/* The reference keeps every update's posterior (RBIS + RBIM, 3.7 KB) in a multimap so that a delayed measurement can
 * be inserted at its timestamp and everything after it re-applied.  Here the posterior of the WHOLE batch after a
 * chosen update is saved device-to-device into one of n_slots checkpoint slots (each = the full state array:
 * 73 MB for 64k 15-state filters -- sized for 288 GB of HBM); the time-ordered bookkeeping and the replay loop live
 * on the host (MavStateEstimator in mav_state_est_batch.hpp).  pb_history_reserve may be called again to resize
 * (contents are lost). */
int pb_history_reserve(pb_ctx *ctx, int n_slots);
int pb_state_save(pb_ctx *ctx, int slot);      /* slot <- head posterior (state, cov, loglik) */
/* Checkpoint without a copy: the NEXT update (pb_predict / pb_update_indexed* / pb_step_legodo) reads the head and
 * writes its posterior straight into checkpoint `slot`, which then IS the head (pb_state_save(slot) becomes a no-op).
 * The step moves the same bytes either way, so a forward pass that keeps every posterior -- what the reference's
 * history does by value (mav_state_est.cpp:55-61) and what the smoother needs -- costs no more than one that keeps none.
 * A saved posterior is never modified afterwards: an update that finds the head in a slot and has no output slot of its
 * own writes back into the context's array; pb_state_restore and pb_reset always land there.  slot = -1 cancels. */
int pb_set_output_slot(pb_ctx *ctx, int slot);
/* The INS posterior of a fused step (EKFSmoothBackwardsPass reads it at every INS update: mav_state_est.cpp:98-189,
 * rbis.cpp:234-266).  One-shot, like pb_set_output_slot: the NEXT pb_step_legodo / pb_step_legodo_split also writes the posterior
 * of its process step -- what pb_predict alone would leave from the same head: bit for bit for 15 states, to rounding
 * (1e-16 relative) for 21 -- into checkpoint `slot`, and consumes the
 * setting whatever its outcome.  pb_step_legodo_correct takes it too, for both correction kinds and with the same contract, when an
 * output slot is pending as well (a checkpointed step: the INS posterior into `slot`, the posterior of the step's last measurement
 * into the output slot -- the two EKFSmoothBackwardsPass reads); with a predicted slot alone it refuses as the calls below.  15 states:
 * ONE launch (k_step_coop_corr_pred); 21 states: the fused step's launch writes the slot and the correction follows as its own launch.  Combines with pb_set_output_slot: one call reads the head and writes two slots.  The filtered
 * posterior is bit-identical to the same call without a predicted slot.  The 15-state two-wave step, the four-wave 21-state step and the
 * two-wave 21-state step (PRONTO_BATCH_QUAD21=0) write both in ONE launch (k_step_quad_pred, k_step_coop_pred); k_step<15> (beyond
 * 393 216 filters) runs the predict into the slot and the fused step as two launches.  PB_ERR_ARG: slot out of range, the pending output slot, or the slot the head lives in.
 * pb_predict, pb_update_indexed*, pb_step_legodo_joints / _feet, pb_run_legodo and pb_replay_legodo_fused /
 * _checkpointed with a predicted slot pending: PB_ERR_STATE (and the setting is cleared).  slot = -1 cancels. */
int pb_set_pred_slot(pb_ctx *ctx, int slot);
/* the checkpoint slot the head currently lives in, or -1 (the context's own array) */
int pb_head_slot(const pb_ctx *ctx);
int pb_state_restore(pb_ctx *ctx, int slot);   /* head posterior <- slot */

/* ekfSmoothingStep (rbis.cpp:234-266), one backward step of MavStateEstimator::EKFSmoothBackwardsPass
 * (mav_state_est.cpp:98-189), on checkpoint slots:
 *   slot_next_pred = posterior of the INS update at k+1 (prediction), slot_next = smoothed (or, for the last step,
 *   filtered) posterior at k+1, slot_cur = filtered posterior at k; slot_out <- smoothed posterior at k.
 * slot_out may be slot_cur (in place) but not one of the k+1 slots.  dt as passed to EKFSmoothBackwardsPass.
 * P^-_{k+1} is factorised WITHOUT the reference's diagonal pivot search (it is SPD; results agree with Eigen's .ldlt() to rounding,
 * tests: <= 1e-9 against the oracle, and as close to exact arithmetic as the pivoted oracle up to a condition number of 1e10).
 * Default kernels: 15 states k_smooth_wide (rbis_smooth_wide.hpp: persistent workgroups, rows through LDS), 21 states k_smooth_lane
 * (rbis_smooth_lane.hpp).  Environment, read by pb_create like every other switch: PRONTO_SMOOTH_KERNEL=lane selects k_smooth_lane for 15 states as well,
 * =reg the kernel of rounds 2-4 (16 / 32 lanes per filter); PRONTO_SMOOTH_PIVOT=1 that kernel with Eigen's pivoting. */
int pb_smooth_step(pb_ctx *ctx, int slot_next_pred, int slot_next, int slot_cur, int slot_out, double dt);

/* Per-filter selection between two posteriors: dst <- src for the filters whose mask entry equals `when` (0 or 1; a non-zero entry
 * counts as 1); every other filter's column of dst is left untouched, bit for bit.  dst / src: checkpoint slots, or PB_SLOT_HEAD = the
 * head posterior (the array it currently lives in: the context's own, or the checkpoint slot an update wrote it into).  Copies every
 * per-filter field of the state array (vec, quat, loglik, packed P).  mask [B]: PB_HOST or PB_DEVICE.  dst == src: no-op.
 * One launch (pb_select.hip): a lane per filter, 16-byte accesses; a filter that is not selected costs its mask byte only.
 * PB_ERR_STATE: a slot out of range (or the head before pb_reset); PB_ERR_ARG: NULL mask, `when` not 0 / 1, `mem` not PB_HOST /
 * PB_DEVICE.  SegmentBatcher (segment_batcher.hpp) keeps every segment's posterior at the end of its own log with it. */
#define PB_SLOT_HEAD (-1)
int pb_slot_select(pb_ctx *ctx, int dst, int src, const uint8_t *mask, int when, int mem);
/* pb_smooth_step for the filters with step[b] = 1; for step[b] = 0 slot_out <- slot_next bit for bit (the filter had no INS update at
 * k+1: its smoothed posterior at k IS its smoothed posterior at k+1).  step: PB_HOST or PB_DEVICE; NULL = all (exactly pb_smooth_step).
 * Why carrying "next" is right: for a filter whose log segment has no INS update at global step k+1, nothing happened to it between
 * k and k+1, so its filtered posterior at k+1 is its filtered posterior at k.  When it has a real update later, at k+2 say, the global
 * step k+1 smooths with cur = posterior(k+1) = posterior(k), predicted = its INS update at k+2 and next = smoothed(k+2): exactly the
 * reference's step from ITS k to ITS next update.  So the carried value, held over the idle ticks, is that filter's correctly smoothed
 * posterior at its own step; an idle tick at the end of its log carries the posterior it ended with (the newest step's "next").
 * pb_smooth_step then pb_slot_select(slot_out, slot_next, step, 0), on the same stream; the smoother kernels are not changed. */
int pb_smooth_step_masked(pb_ctx *ctx, int slot_next_pred, int slot_next, int slot_cur, int slot_out, double dt, const uint8_t *step,
                          int mem);

/* EKFSmoothBackwardsPass over a WHOLE log with bounded memory (mav_state_est.cpp:98-189, lcm_front_end.cpp:168-203: the reference's
 * "-S" smooths the entire log; it keeps three posteriors per step by value, which for a batch is 2 T slots of the whole state).
 * Checkpoint and recompute: the forward pass filters the n_steps steps of the streams (as pb_run_legodo takes them; per step the
 * process step, then the velocity update -- the per-message kernels of pb_predict / pb_update_indexed) from the current head and
 * keeps only the posterior in front of every `stride`-th step; the backward pass re-runs the log stretch by stretch, newest
 * first, into a window of 2 * stride slots and applies pb_smooth_step to every step but the newest.  It uses the checkpoint slots
 * [first_slot, first_slot + pb_smooth_log_slots(n_steps, stride)) = n_steps / stride + 2 * stride + 4 slots instead of 2 * n_steps
 * (stride near sqrt(n_steps / 2) is the minimum).  sink(user, step, slot) is called, newest step first, once the smoother step
 * of `step` has been ENQUEUED: `slot` holds the smoothed posterior of that step until the NEXT call of the sink returns; read it with
 * stream-ordered calls that leave the head alone (pb_get_slot, pb_snapshot_from_slot).  The smoothed posteriors are, bit for bit,
 * those of the all-checkpoints pass (pb_set_output_slot per update + pb_smooth_step).  Afterwards the head is the newest filtered
 * posterior.  dt as pb_smooth_step.  elapsed_ms != NULL: device time of the whole call (forward + backward). */
typedef void (*pb_smooth_sink)(void *user, int step, int slot);
int pb_smooth_log_slots(int n_steps, int stride);
int pb_smooth_log(pb_ctx *ctx, int n_steps, int stride, const double *imu_stream, const double *lo_stream, const uint8_t *mask_stream,
                  const double q[4], double dt, int first_slot, pb_smooth_sink sink, void *user, float *elapsed_ms);
/* pb_smooth_log on the fused step: same arguments, slots (pb_smooth_log_slots), sink order, head afterwards and elapsed_ms.  Every
 * step of the forward and recompute passes is ONE launch with the semantics of pb_step_legodo (two state round trips per recomputed
 * step instead of four: in the recompute pass that launch writes the window's predicted slot, pb_set_pred_slot, and its filtered slot,
 * pb_set_output_slot, together).  The smoothed posteriors are, bit for bit, those of the all-checkpoints pass built from
 * pb_set_pred_slot + pb_set_output_slot + pb_step_legodo + pb_smooth_step, and agree with pb_smooth_log to rounding (the fused
 * kernel and the two per-message kernels round differently); the head afterwards is bit-identical to n_steps pb_step_legodo calls.
 * On an error the head is back in the context's own array (the pre-call head, or the newest posterior once the forward pass is
 * over) and no output / predicted slot is pending. */
int pb_smooth_log_fused(pb_ctx *ctx, int n_steps, int stride, const double *imu_stream, const double *lo_stream, const uint8_t *mask_stream,
                        const double q[4], double dt, int first_slot, pb_smooth_sink sink, void *user, float *elapsed_ms);

/* pb_smooth_log / pb_smooth_log_fused for a log with a sparse stream of corrections behind some of its IMU + leg-odometry pairs: the
 * 6-DoF visual-odometry position_orient (PB_CORR_POS_ORIENT) or the scan-match position_yaw (PB_CORR_POS_YAW) of
 * pb_step_legodo_correct.  EKFSmoothBackwardsPass takes as "cur" the posterior of the LAST measurement behind an INS update
 * (mav_state_est.cpp:98-189), however many there were; so the step's filtered posterior is the one behind its correction.
 * A step with a tick: fused = 1, one pb_step_legodo_correct (in the recompute pass with the window's predicted and filtered slots
 * set: one launch for 15 states, two for 21); fused = 0, pb_predict, pb_update_indexed and pb_update_indexed_orient into the same
 * filtered slot -- the per-message kernels.  A step without a tick is the step of pb_smooth_log_fused / pb_smooth_log.  Slots
 * (pb_smooth_log_slots), sink order, head afterwards, error contract and elapsed_ms are theirs; corr == NULL or n_ticks == 0 IS
 * pb_smooth_log_fused / pb_smooth_log, bit for bit.  The recompute pass re-applies the same correction blocks, so the smoothed
 * posteriors are, bit for bit, those of the all-checkpoints pass built from the same calls (fused: pb_set_pred_slot +
 * pb_set_output_slot + pb_step_legodo_correct + pb_smooth_step); fused and un-fused agree to the rounding stated at
 * pb_step_legodo_correct.  PB_ERR_ARG, the head left usable in the context's own array: an unknown kind, a step list that is not
 * strictly increasing or leaves [0, n_steps), NULL step / z2 / R2 / quat_meas2 with n_ticks > 0, an R2 that is not diagonal.
 * position_orient: the measurement is the caller's COMPOSED pose T1 = T0 o delta, and T0 depends on the filter's posterior at the key
 * frame (rbis_fovis_update.cpp:184-223): the blocks come from a forward run (pb_snapshot* / pb_compose_delta) or from a synthetic
 * stream; this call composes nothing.  A scan-match position_yaw is absolute and needs no such step. */
typedef struct pb_corr_stream {
  int kind;                  /* PB_CORR_POS_ORIENT | PB_CORR_POS_YAW; m = 6 | 4 */
  int n_ticks;               /* 0 is allowed */
  const int32_t *step;       /* HOST int32[n_ticks], strictly increasing, each in [0, n_steps): the correction
                                follows the IMU + leg-odometry pair of that step */
  const double *z2;          /* device [n_ticks][m][B] */
  const double *R2;          /* device [n_ticks][m][B] (PB_R_DIAG) or host double[m] (PB_R_DIAG_BROADCAST) */
  int r_kind2;
  const double *quat_meas2;  /* device [n_ticks][4][B] */
  const uint8_t *mask2;      /* device [n_ticks][B] or NULL */
} pb_corr_stream;
int pb_smooth_log_corrected(pb_ctx *ctx, int n_steps, int stride, const double *imu_stream, const double *lo_stream,
                            const uint8_t *mask_stream, const double q[4], double dt, int first_slot, const pb_corr_stream *corr,
                            int fused, pb_smooth_sink sink, void *user, float *elapsed_ms);

/* ---- accuracy against ground truth (motion_estimate/scripts/drift_per_distance.py) ------------------------------------------
 * The reference judges an estimator by comparing POSE_BODY with POSE_GROUND_TRUTH (Vicon): between two ground-truth messages
 * more than parameterTimeElapsedThreshold apart it compares the RELATIVE motion of the estimate with that of the truth and
 * publishes pronto::error_metrics_t on PRONTO_ERROR.  Here every filter of the batch keeps the script's State
 * (the anchor ground-truth pose `last`, the anchor estimate `last_est`) and accumulators next to its filter state, and one kernel
 * launch per ground-truth message (one lane per filter, about 0.5 KB per filter) replaces the flush + pb_get_head + host loop a
 * caller needs otherwise.  Scoring reads the filter's position (state rows 9..11) and quaternion and writes nothing of the filter:
 * head, history and log-likelihood are unchanged bit for bit, and a pending pb_set_output_slot / pb_set_pred_slot stays pending.
 * Quaternions are w, x, y, z and are not normalised, as in the script (botpy.py:30-88).
 *
 * Drift windows (PB_SCORE_DRIFT), per filter with a valid message (drift_per_distance.py:70-138):
 *   no anchor yet (anchor utime < 0, :79)   last <- (utime, pos, q), last_est <- the filter's estimate; nothing else
 *   otherwise  dist = |pos - last.pos| (:60); the window closes when (double)(utime - last.utime) > time_threshold_s * 1e6 (the
 *              script's strict comparison, :65), or when distance_threshold > 0 and dist > distance_threshold (the test the script
 *              carries commented out, :62-63; 0 = off = the script as it ships)
 *   on closing gt_ab = inv(last) o (pos, q), se_ab = inv(last_est) o estimate (botpy.transform_relative), and error_metrics_t:
 *              pos_error = se_ab.t - gt_ab.t, pos_error_norm, rpy_error = [0, 0, yaw(se_ab) - yaw(gt_ab)] in degrees, NOT wrapped
 *              (:107-109), distance_travelled = dist, percent_ddt = 100 pos_error_norm / dist -- the IEEE quotient: inf or NaN
 *              when the truth did not move (:104) --, utime = utime, and
 *              time_elapsed = (last.utime - utime) * 1e-6, which is NEGATIVE: the script subtracts the wrong way round (:131) and
 *              its sign is kept.  Then last <- (utime, pos, q), last_est <- estimate (:136-137).
 * Absolute error (PB_SCORE_ABS; an addition, the script has none): at every valid message, whatever the order of the messages,
 * e = estimate.pos - pos and the yaw difference wrapped into (-180, 180] degrees.  It is the supported way to score smoothed
 * posteriors (an explicit `slot`), whose newest-first order gives other drift windows.
 */
enum pb_score_flags { PB_SCORE_DRIFT = 1, PB_SCORE_ABS = 2 };
/* rows of the per-filter score state, doubles (pb_score_get rows_out) */
enum pb_score_row {
  PB_SCORE_ANCHOR_GT = 0,             /* 7 rows: `last` pos[3], orientation[4] (w, x, y, z)                                  */
  PB_SCORE_ANCHOR_EST = 7,            /* 7 rows: `last_est` pos[3], orientation[4]                                           */
  PB_SCORE_LAST_POS_ERROR = 14,       /* the newest window's error_metrics_t, in the message's field order (10 rows):        */
  PB_SCORE_LAST_POS_ERROR_NORM = 17,  /*   pos_error[3], pos_error_norm [m],                                                 */
  PB_SCORE_LAST_RPY_ERROR = 18,       /*   rpy_error[3] [deg] (roll and pitch always 0, yaw not wrapped),                    */
  PB_SCORE_LAST_DISTANCE = 21,        /*   distance_travelled [m],                                                           */
  PB_SCORE_LAST_PERCENT_DDT = 22,     /*   percent_ddt (non-finite when distance_travelled = 0),                             */
  PB_SCORE_LAST_TIME_ELAPSED = 23,    /*   time_elapsed [s], NEGATIVE (the script's sign)                                    */
  PB_SCORE_SUM_ERR = 24,              /* sum of pos_error_norm over the closed windows                                       */
  PB_SCORE_SUM_ERR_SQ = 25,           /* sum of pos_error_norm^2                                                             */
  PB_SCORE_MAX_ERR = 26,              /* largest pos_error_norm                                                              */
  PB_SCORE_SUM_DISTANCE = 27,         /* sum of distance_travelled                                                           */
  PB_SCORE_SUM_TIME = 28,             /* sum of |time_elapsed|                                                               */
  PB_SCORE_SUM_YAW_SQ = 29,           /* sum of (rpy_error[2] wrapped into (-180, 180])^2                                    */
  PB_SCORE_SUM_PDDT = 30,             /* sum of percent_ddt over the windows with distance_travelled > 0 (PB_SCORE_N_DDT)    */
  PB_SCORE_MAX_PDDT = 31,             /* largest percent_ddt of those windows                                                */
  PB_SCORE_ABS_SUM_SQ = 32,           /* PB_SCORE_ABS: sum of |estimate.pos - pos|^2                                         */
  PB_SCORE_ABS_MAX = 33,              /* PB_SCORE_ABS: largest |estimate.pos - pos|                                          */
  PB_SCORE_ABS_SUM_YAW_SQ = 34,       /* PB_SCORE_ABS: sum of (yaw(estimate) - yaw(truth) wrapped into (-180, 180] deg)^2    */
  PB_SCORE_ROWS = 35
};
/* rows of the per-filter score state, 64-bit integers (pb_score_get counts_out) */
enum pb_score_count {
  PB_SCORE_ANCHOR_UTIME = 0,  /* last.utime; -2 = no anchor yet (State.__init__, drift_per_distance.py:31) */
  PB_SCORE_LAST_UTIME = 1,    /* utime of the newest window's error_metrics_t; -2 = no window yet            */
  PB_SCORE_N_WINDOWS = 2,     /* closed windows                                                              */
  PB_SCORE_N_DDT = 3,         /* closed windows with distance_travelled > 0                                  */
  PB_SCORE_ABS_N = 4,         /* PB_SCORE_ABS messages                                                       */
  PB_SCORE_COUNTS = 5
};
/* what pb_score_best ranks by; a filter with no window (with distance > 0) / no PB_SCORE_ABS message has no data for it */
enum pb_score_metric {
  PB_SCORE_MEAN_PDDT = 0,  /* PB_SCORE_SUM_PDDT / PB_SCORE_N_DDT: mean percent drift per distance travelled   */
  PB_SCORE_RMS_DRIFT = 1,  /* sqrt(PB_SCORE_SUM_ERR_SQ / PB_SCORE_N_WINDOWS) [m]                              */
  PB_SCORE_ATE_RMSE = 2    /* sqrt(PB_SCORE_ABS_SUM_SQ / PB_SCORE_ABS_N) [m]: absolute trajectory error       */
};
/* State.__init__ (drift_per_distance.py:25-40) for every filter: allocates the score state on the first call, clears it on every
 * call (again = reset).  time_threshold_s: parameterTimeElapsedThreshold (10.0 in the script); distance_threshold:
 * parameterDDTThreshold (0.25 in the script, unused there), 0 = off.  PB_ERR_ARG: a negative or NaN threshold. */
int pb_score_init(pb_ctx *ctx, double time_threshold_s, double distance_threshold);
/* on_pose_gt (drift_per_distance.py:70-138) for every filter, with most_recent_est (on_pose_est, :53-56) = the filter's position and
 * quaternion as they are in `slot`: PB_SLOT_HEAD = wherever the head lives now (the context's own array, or the checkpoint slot an
 * update wrote it into), else a checkpoint slot.  pose7 = pos[3], orientation[4]: [7][B] (PB_HOST, PB_DEVICE) or [7] host values for
 * every filter (PB_HOST_BROADCAST: one robot's truth for a whole sweep; kernel arguments, nothing of batch size is moved).
 * utimes [B] or NULL: per-filter message times instead of utime; valid [B] or NULL: 0 = this filter has no message, it costs the read
 * of its byte and nothing else.  Both live where pose7 lives (host for PB_HOST_BROADCAST).  flags: PB_SCORE_DRIFT | PB_SCORE_ABS,
 * at least one.  One launch on the context's stream; nothing is synchronised beyond the copy of PB_HOST inputs.
 * PB_ERR_STATE: before pb_reset or pb_score_init, slot out of range.  PB_ERR_ARG: NULL pose7, unknown flags or mem. */
int pb_score_ground_truth(pb_ctx *ctx, int64_t utime, const int64_t *utimes, const double *pose7, const uint8_t *valid, int slot,
                          int flags, int mem);
/* the score state of filters [first, first + count): rows_out [PB_SCORE_ROWS][count] doubles, counts_out [PB_SCORE_COUNTS][count]
 * 64-bit integers, either may be NULL; mem PB_HOST (synchronises) or PB_DEVICE. */
int pb_score_get(pb_ctx *ctx, int first, int count, double *rows_out, int64_t *counts_out, int mem);
/* the newest error_metrics_t of one filter (what the script publishes on PRONTO_ERROR, :124-133), host: *utime (-2: no window yet) and
 * out[10] in the message's field order: pos_error[3], pos_error_norm, rpy_error[3], distance_travelled, percent_ddt, time_elapsed
 * (negative, see above).  Synchronises. */
int pb_score_last(pb_ctx *ctx, int filter, int64_t *utime, double out[10]);
/* the filter with the smallest `metric` (enum pb_score_metric) among the filters that have data for it, found on the device (two
 * launches); on a tie the lowest filter index.  A filter whose metric is NaN counts as without data.  No filter with data:
 * *filter_out = -1 and *value_out = 0.  value_out may be NULL.  Synchronises.  Replaces the log-likelihood ranking a sweep had to
 * fall back on (examples/param_sweep.c) by the reference's own accuracy measure. */
int pb_score_best(pb_ctx *ctx, int metric, int *filter_out, double *value_out);

/* ---- estimator queries (mav_state_est.hpp:20-22) -------------------------------------------------------- */

/* MavStateEstimator::getHeadState + getMeasurementsLogLikelihood for filters [first, first+count):
 * vec_out [n][count], quat_out [4][count], cov_out [n*n][count] full column-major (as rbis.cpp:300 Map<RBIM>),
 * ll_out [count]; any of them may be NULL. */
int pb_get_head(pb_ctx *ctx, int first, int count, double *vec_out, double *quat_out, double *cov_out,
                double *ll_out, int mem);
/* rbisCreateFilterStateMessageCPP (rbis.cpp:287-304) for one filter: quat[4], state[21], cov[441] (host). */
/* the same read of a posterior that lives in checkpoint slot `slot` (the head stays what it is) */
int pb_get_slot(pb_ctx *ctx, int slot, int first, int count, double *vec_out, double *quat_out, double *cov_out, double *loglik_out,
                int mem);
int pb_get_filter_state(pb_ctx *ctx, int filter, double quat[4], double state[21], double cov[441]);
/* per-shard run summary for the end-of-run all-reduce:
 * out[0] = sum loglik, out[1] = sum |vec| + |quat| (checksum), out[2] = max | |quat|^2 - 1 |,
 * out[3] = number of non-finite state entries. */
int pb_summary(pb_ctx *ctx, double out[4]);
/* How many filters a DEVICE-resident update mask [B] lets through (synchronises).  The reference's handlers return NULL when a
 * message yields no update (rbis_legodo_update.cpp:242-255, rbis_fovis_update.cpp:160-164), so such a message never enters the
 * history; a batched handler whose per-filter validity is decided on the device cannot know that when it returns.  The shim asks
 * lazily -- only where the difference is observable: FovisHandler's history.updateMap.lower_bound look-up
 * (rbis_fovis_update.cpp:184-207) skips updates that applied to no filter. */
int pb_mask_count(pb_ctx *ctx, const uint8_t *mask_dev, int *count_out);
/* Bit-level checksum of the whole device state (every component of every filter, padding lanes of the last tile included):
 * out[0] a weighted wrapping sum, out[1] a xor of rotated words; slot < 0 = the head, else a checkpoint slot.  Two runs of
 * the same context over the same inputs must give the same pair (tests: replay identity over thousands of launches);
 * one pass over the state, ~15 us at 64k filters. */
int pb_state_checksum(pb_ctx *ctx, int slot, uint64_t out[2]);
/* Measurement aid (not on the reference path): `reps` plain copies of the whole state array with the step kernels' exact
 * access pattern (one tile row = 64 lanes x 16 bytes per buffer_load / buffer_store_dwordx4), to calibrate rocprofv3's
 * FETCH_SIZE / WRITE_SIZE on a known byte count and to measure this box's achievable copy rate.  elapsed_ms = HIP-event
 * time of the reps.  pb_calib_copy_checksum: the same copies, then pb_state_checksum's pair OF THE COPY (must equal the
 * head's: the regression test of the 16-byte store path, tests/test_gpu_edge_cases.py). */
int pb_calib_copy(pb_ctx *ctx, int reps, float *elapsed_ms);
int pb_calib_copy_checksum(pb_ctx *ctx, int reps, uint64_t out[2]);
/* head utime bookkeeping (posterior_state.utime = update->utime, mav_state_est.cpp:60) */
int pb_set_utime(pb_ctx *ctx, int64_t utime);
int64_t pb_get_utime(const pb_ctx *ctx);

/* ---- Gaussian particle filter measurement (state-estimator/src/gpf/gpf.hpp:53-192, rbis_gpf_update.cpp:28-76) -------
 * The front half of a GPF update for every filter of the batch: draw K states from the marginal of the rows idx (m = 1..9,
 * distinct, inside the state), score them, fit the weighted and the unweighted cloud, solve for the effective measurement.
 * The outputs z_eff [m][B] / R_eff [m*m][B] are exactly the blocks pb_update_indexed_wide(..., PB_R_FULL, ..., PB_DEVICE)
 * takes: applying them is that call's.  All blocks are device memory, [rows][B] doubles; sample-indexed blocks are
 * [K][rows][B].  None of these calls writes the filter or takes a pending pb_set_pred_slot / pb_set_output_slot.
 * PB_ERR_ARG: m outside 1..9, repeated or out-of-range indices, K < 1, a NULL block, a grid call before pb_gpf_grid_set. */

/* [rows][B] standard normals, counter-based (no state in the context: any (filter, row) can be reproduced).
 * Philox4x32-10 with key (seed low, seed high) and counter (filter b, row pair j = row / 2, stream_id, 0); from its words
 * w0..w3: u1 = (((w0 2^32 + w1) >> 11) + 0.5) 2^-53, u2 likewise from w2, w3; row 2j = sqrt(-2 ln u1) cos(2 pi u2),
 * row 2j + 1 = sqrt(-2 ln u1) sin(2 pi u2). */
int pb_gpf_normals(pb_ctx *ctx, uint64_t seed, uint32_t stream_id, int rows, double *out_dev);
/* xi [K][m][B] (standard normals) -> delta [K][m][B], s_k = L xi_k with L the lower Cholesky factor of P[idx, idx]
 * (gpf.hpp:68-94), and pose [K][7][B]: position xyz then quaternion wxyz of the head with vec[idx_i] += s_k[i] and chi
 * folded into the quaternion under the context's tolerance (gpf.hpp:97-103; what RBIS::getBotTrans hands a likelihood).
 * A filter whose P[idx, idx] is not positive definite: delta = 0, every sample is the head, the fit reports status 2. */
int pb_gpf_sample(pb_ctx *ctx, int m, const int *idx, int K, const double *xi_dev, double *delta_out_dev, double *pose_out_dev);
/* delta [K][m][B], loglik [K][B] -> z_eff [m][B], R_eff [m*m][B] column-major, status int32 [B] (gpf.hpp:106-200):
 * w_k = exp(l_k - max l), W = sum w_k.  Unless 5 m < W < max_weight_proportion K (both strict): R_eff = 1e4 I,
 * z_eff = x[idx], status 2.  Otherwise (mean, cov) of the samples with unit weights (u) and with w (cov = sum w (x - mean)
 * (x - mean)^T / sum w, no K - 1 correction); R_eff = (C_w^-1 - C_u^-1)^-1; z_eff = x[idx] + K_eff^-1 (mean_w - mean_u) with
 * K_eff^T = (P[idx, idx] + R_eff)^-1 C_u; then the eigenvalues of R_eff below zero are set to 1e4 (status 1, else 0).
 * Status 2 also for a filter with a non-finite loglik or a cloud whose covariance is not positive definite.  Bit-identical
 * from run to run. */
int pb_gpf_measurement(pb_ctx *ctx, int m, const int *idx, int K, const double *delta_dev, const double *loglik_dev,
                       double max_weight_proportion, double *z_eff_out_dev, double *R_eff_out_dev, int32_t *status_out_dev);
/* The built-in likelihood: evaluateScanLogLikelihood + evaluatePointLogLikelihood (LaserLikelihoodInterface.cpp:5-77) over a
 * dense voxel grid in place of the octomap.  values_host double [nz][ny][nx] (dims = nx, ny, nz): what
 * -node->getLogOdds() would return; copied, the array is free on return.  resolution, cov_scaling > 0. */
int pb_gpf_grid_set(pb_ctx *ctx, const double origin[3], double resolution, const int dims[3], const double *values_host,
                    double unknown_loglike, double cov_scaling);
/* pose [K][7][B] (pb_gpf_sample) -> loglik [K][B].  points: n_points body-frame points, rows x0, y0, z0, x1, ...:
 * [3 n_points][B] (PB_DEVICE, PB_HOST) or [3 n_points] host doubles (PB_HOST_BROADCAST: one robot's scan for every
 * filter).  Per sample and point: p_map = R(q) p + t; a coordinate below origin or above origin + dims resolution scores
 * unknown_loglike, else the voxel min((int) floor((c - origin_c) / resolution), dim_c - 1) per axis; loglik = sum /
 * cov_scaling.  A point whose x is not finite is skipped (the reference's point_status filter). */
int pb_gpf_grid_loglik(pb_ctx *ctx, int K, const double *pose_dev, int n_points, const double *points, int points_mem,
                       double *loglik_out_dev);

/* ---- Optical-flow sigma-point update (RBISOpticalFlowMeasurement, rbis_update_interface.cpp:109-260) -----------------
 * The reference's one nonlinear measurement z = h(x): four rows (ux, uy, theta, scale) of a camera looking at the ground,
 * taken by an unscented update with the reference's hard-coded weights (a2 = 1e-6, b = 2, k = 0, n = 21; :199-206).  One
 * launch per message; h reads rows 0 ... 11 of the state only, so the update factors twelve columns of P and evaluates h 25
 * times where the reference takes 43 sigma points off the full factor -- algebraically the same update. */

/* The camera, once per context (OpticalFlowHandler's constructor, sensor_handlers.cpp:726-731): body_to_cam_trans is r, and
 * zeta1, zeta2, eta are what RBISOpticalFlowMeasurement's constructor takes (rbis_update_interface.hpp:146-148): the COLUMNS
 * of the Eigen matrix that bot_trans_get_rot_mat_3x3 filled row-major, i.e. the ROWS of libbot's body -> camera rotation. */
int pb_flow_set_camera(pb_ctx *ctx, const double body_to_cam_trans[3], const double zeta1[3], const double zeta2[3],
                       const double eta[3]);
/* flags bit 0: the orientation h sees is quat_head * Exp(chi_sigma) (what addState would give).  Default 0 is the reference:
 * RBIS(state_vec) of :113 starts from the identity, so the orientation is Exp(chi_sigma) where |chi_sigma| exceeds the fold
 * tolerance of pb_set_constants and the identity otherwise; the head's quaternion does not enter. */
#define PB_FLOW_HEAD_QUAT 1
/* RBISOpticalFlowMeasurement::updateFilter (:160-260) with measure (:111-138) for every filter.
 * flow_block [7][B] (or [7] host doubles under PB_HOST_BROADCAST): ux, uy, theta, scale -- z_meas, sensor_handlers.cpp:748-751
 * -- then alpha1, alpha2, gamma (:753-755).  R is 4 x 4 in the three pb_rkind encodings, as for pb_update_indexed (the
 * handler's is diag(r_ux, r_uy, r_r, r_s)^2, :735-742).  mask [B] uint8 or NULL; mem = PB_HOST, PB_DEVICE or
 * PB_HOST_BROADCAST (broadcast: mask must be NULL), as for pb_update_indexed_wide.  pb_set_output_slot is honoured, a pending
 * pb_set_pred_slot is refused; PB_ERR_STATE before pb_flow_set_camera.
 * As in the reference the posterior is the prior with vec += K (z_meas - zhat), NOT folded (:257; the next predict's addState
 * folds chi), P -= K Pzz K^T (:258); the quaternion and the log-likelihood keep the prior's bits (:163,190).  Pzz is factored
 * by the unpivoted LDL^T of the other updates (:254).  There is no guard on the height term (:191-192 is commented out):
 * non-finite results show up in pb_summary.
 * zhat_out DEVICE [4][B] or NULL: the predicted measurement the reference publishes as OPTICAL_FLOW_PSEUDO (:140-158,236);
 * written for the filters with status 0 only.
 * status_out DEVICE int32 [B] or NULL: 0 applied; 1 masked off; 2 + k: pivot k (0 ... 11) of the Cholesky factor of P is not
 * positive or not finite -- the filter keeps its state bit for bit.  (The reference returns only when the factor holds a
 * NaN and otherwise goes on with what Eigen's failed LLT left behind, :211-217; that is not imitated.) */
int pb_update_optical_flow(pb_ctx *ctx, const double *flow_block, const double *R, int r_kind, const uint8_t *mask, int mem,
                           int flags, double *zhat_out, int32_t *status_out);

/* library identification: "pronto_batch <version> gfx950" */
const char *pb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PRONTO_BATCH_H */
