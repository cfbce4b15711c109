// pb_ctx.hpp -- the context behind the C ABI, the owner of its device memory (dev_alloc / dev_release) and what crosses the translation
// units of libpronto_batch.so: the per-call guard, the input resolver and the launchers.  It includes the
// argument types of the kernels (rbis_tile_io.hpp, rbis_coop.hpp, rbis_legodo.hpp, rbis_jointfilt.hpp, rbis_yawlock.hpp, rbis_score.hpp, rbis_gpf.hpp, rbis_flow.hpp), never a kernel: each .hip
// includes the kernel headers it launches from, so every kernel is compiled in one object.  WHICH kernel a launcher runs is decided in
// pb_policy.hpp (host-only, tested on the CPU): the context keeps one Policy, made in pb_create.
// (the kernels are instantiated in twenty-four objects so that they compile in parallel, see the Makefile: pb_step.hip, pb_step_pred.hip,
// pb_step_corr_pred.hip, pb_step_leg.hip and pb_legpar.hip -- one object per state size -- the step kernels; pb_update.hip, pb_update_rt21.hip -- three objects, by m --,
// pb_update_ct.hip and pb_update_wide.hip (seven to nine rows, with its entry point pb_update_indexed_wide) the update kernels; pb_smooth.hip and pb_smooth_wide.hip the smoother; pb_select.hip.  A family's kernels, launchers
// and entry points of the C ABI share one unit: pb_legodo.hip leg odometry and joint filters, pb_yawlock.hip, pb_frontend.hip the IMU
// front end, pb_score.hip the ground-truth scorer, pb_gpf.hip the GPF measurement, pb_flow.hip the optical-flow update; pb_history.hip the checkpoint slots and whole-log smoothing, which launches through
// pbk_* only; pronto_batch.hip the context, staging, steps, updates and read-back).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/pronto_batch.h"
#include "pb_policy.hpp"
#include "rbis_tile_io.hpp"
#include "rbis_coop.hpp"
#include "rbis_legodo.hpp"
#include "rbis_jointfilt.hpp"
#include "rbis_yawlock.hpp"
#include "rbis_score.hpp"
#include "rbis_gpf.hpp"
#include "rbis_flow.hpp"

using namespace pb;

#define PB_MAX_FENCES 16

struct pb_ctx {
  int ns = 0, B = 0, dev = 0, nsnap = 0, nc = 0;  // nc: canonical components (Lay<NS>::NC)
  long stride = 0;      // batch rounded up to whole 64-filter tiles
  size_t state_doubles = 0;  // one state array / checkpoint slot: stride * Slots<NS>::NSLOT (tiled layout)
  hipStream_t stream = nullptr, own_stream = nullptr;
  double *st = nullptr;       // the HEAD posterior: st_base, or a checkpoint slot an update wrote its posterior into
  double *st_base = nullptr;  // the context's own state array
  int out_slot = -1;          // pb_set_output_slot: where the next update writes (then that slot is the head)
  int pred_slot = -1;         // pb_set_pred_slot: where the next fused step also writes its predicted posterior (one-shot)
  double *snaps = nullptr, *d_small = nullptr;
  double *hist = nullptr;  // posterior checkpoint slots (pb_history_reserve)
  int nhist = 0;
  double *legd = nullptr;   // leg odometry state (pb_legodo_init): [NLD][stride] doubles ...
  int64_t *legi = nullptr;  // ... and [NLI][stride] 64-bit integers (rbis_legodo.hpp)
  LegPar leg_par;
  int64_t *leg_ut = nullptr;      // per-filter message times / validity of the NEXT odometry call (pb_legodo_set_message_times),
  uint8_t *leg_valid = nullptr;   // device [B] each; consumed by that call
  bool leg_ut_on = false, leg_valid_on = false;
  const int64_t *leg_ut_ext = nullptr;    // PB_DEVICE times / validity are read in place: the caller's arrays, not copies
  const uint8_t *leg_valid_ext = nullptr;
  double *leg_blk = nullptr;      // pb_legodo_set_param_block: the odometry's noises and contact thresholds per filter, [PB_LEGPAR_ROWS][stride]
  bool leg_blk_on = false;        // ... in force: the kernels read it instead of leg_par.alt / total_force / level and the calls' noises
  LegMeasPar leg_meas;            // pb_legodo_set_measurement_mode: which of LegOdoCommon's measurements the odometry calls write
  LegChain *leg_chain = nullptr;  // forward-kinematics chain table (pb_legodo_set_chain), device copy ...
  LegChain leg_chain_h;           // ... and the host copy (PB_HOST_BROADCAST joint states are reduced to chain angles on the host)
  int leg_chain_rows = 0;         // rows a joint-position block must have (highest row the chain reads + 1)
  int32_t *leg_nc = nullptr;      // controller contact counts [2][B] (pb_legodo_set_control_contacts), used when leg_nc_dev
  int leg_nc_h[2] = { -1, -1 };   // ... or ONE pair for every filter (-1: none received yet)
  bool leg_nc_dev = false;
  // joint-position filters in front of the kinematics (pb_joint_filter_init / pb_joint_filter, rbis_jointfilt.hpp)
  JfPar jf_par;
  bool jf_ready = false, jf_first = true;
  int jf_input = -1;              // -1 no message yet, 0 per-robot blocks (state in HBM), 1 one robot (state on the host)
  int jf_head = 0;                // low-pass window slot of the oldest sample
  double jf_tlast = 0;            // SimpleKalmanFilter::tlast_
  float *jf_ring = nullptr;       // [JF_TAPS][nf][B] floats
  double *jf_kst = nullptr;       // [JF_KSTATE][nf][B]
  std::vector<float> jf_ring_h;   // [JF_TAPS][nf]   (one robot)
  std::vector<double> jf_kst_h;   // [JF_KSTATE][nf]
  double *leg_lo = nullptr;       // measurement block + mask between the two kernels of pb_step_legodo_joints' fallback path
  // yaw lock (pb_yawlock_init, rbis_yawlock.hpp): per-filter state [NYD][stride] doubles + [NYI][stride] 64-bit words
  YawPar yaw_par;
  double *yawd = nullptr;
  int64_t *yawi = nullptr;
  uint8_t *yaw_standing = nullptr;  // what the status / IMU handlers keep (pb_yawlock_set_standing / _set_gyro): [stride] device
  double *yaw_gyro = nullptr;       // arrays, used when the matching *_dev is set, or ONE value for every filter
  bool yaw_standing_dev = false, yaw_gyro_dev = false;
  int yaw_standing_all = 0;
  double yaw_gyro_all = 0.0;
  // drift per distance against ground truth (pb_score_init, rbis_score.hpp): per-filter state [PB_SCORE_ROWS][stride] doubles +
  // [PB_SCORE_COUNTS][stride] 64-bit words
  ScorePar score_par;
  double *scored = nullptr;
  int64_t *scorei = nullptr;
  // the GPF's built-in likelihood (pb_gpf_grid_set, rbis_gpf.hpp): the voxel values [nz][ny][nx] and one robot's scan points [3 n]
  GpfGrid gpf_par;
  double *gpf_grid = nullptr, *gpf_pts = nullptr;
  size_t gpf_grid_n = 0, gpf_pts_n = 0;
  bool gpf_grid_on = false;
  // the optical-flow update (pb_flow_set_camera, rbis_flow.hpp): the camera and the reference's five sigma-point weights
  FlowCam flow_cam;
  FlowWeights flow_wt;
  bool flow_cam_on = false;
  double *notch = nullptr;  // IMU notch cascade state [36][stride] (pb_imu_notch_init)
  NotchCoef notch_coef;
  bool notch_ready = false;
  // IMU front end per filter (pb_ins_body_block, rbis_frontend.hpp): last body-frame sample [6][stride], previous message time [stride]
  double *ins_last = nullptr;
  int64_t *ins_prev_ut = nullptr;
  const uint8_t *imu_valid_next = nullptr;   // pb_set_imu_valid: one-shot, taken by the next call that takes an IMU step (Call) ...
  const uint8_t *imu_valid_cur = nullptr;    // ... and held here for the duration of that call
  double *imu_keep = nullptr;                // [7][B]: the IMU block that call's step kernel reads instead (pbk_idle_prepare), and behind
                                             // it [12][B]: the idle filters' omega / acceleration covariance blocks (pbk_idle_restore)
  const uint8_t *imu_idle_cur = nullptr;     // the mask pbk_idle_prepare applied in this call: its step launches are followed by pbk_idle_restore
  // chunked uploads (pb_upload_async): fences recorded on the main stream, one event for "the uploads issued so far"
  hipEvent_t fence[PB_MAX_FENCES] = {};
  int n_fences = 0;
  hipEvent_t ev_upload = nullptr;
  void *stage = nullptr;
  size_t stage_bytes = 0;
  // PB_HOST inputs: two staging buffers filled on a copy stream, so that the copy of message k+1 overlaps the kernels
  // of message k (with pinned source buffers, pb_host_alloc, the DMA runs at link rate)
  void *in_stage[2] = { nullptr, nullptr };
  size_t in_stage_bytes[2] = { 0, 0 };
  int in_idx = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_consumed[2] = { nullptr, nullptr }, ev_copied = nullptr;
  Consts k{ 9.80665, 1e-6 };
  int64_t utime = 0;
  bool have_state = false;
  Policy policy;  // which kernel, grid shape and cache policy this context runs (pb_policy.hpp; made once, in pb_create)
  bool smooth_attr = false;  // dynamic-LDS limit of the smoother kernels raised on this device
  bool smooth_wide_attr = false;
  int n_cu = 256;            // compute units of the device (grid of the persistent smoother kernel)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void *> owned;  // every device allocation behind the pointers above (dev_alloc / dev_release); pb_destroy frees these
  char err[512] = { 0 };
};

inline thread_local char g_create_err[512] = "";

inline int fail(pb_ctx *c, int code, const char *fmt, ...)
{
  char *dst = c ? c->err : g_create_err;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(dst, 512, fmt, ap);
  va_end(ap);
  return code;
}

#define HIPCHK(c, call)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) return fail((c), PB_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

inline int nblk(int n) { return (n + 63) / 64; }

// ---- the context's device memory: one owner ----
// Every device buffer a pb_ctx member points to is allocated here and recorded in c->owned, which pb_destroy frees; no family keeps a
// free list of its own.  `count` elements of T (bytes for a void pointer); nothing happens when p is set already.
template <class T>
hipError_t dev_alloc_hip(pb_ctx *c, T *&p, size_t count)
{
  if (p) return hipSuccess;
  void *mem = nullptr;
  hipError_t e = hipMalloc(&mem, sizeof(std::conditional_t<std::is_void_v<T>, char, T>) * count);
  if (e != hipSuccess) return e;
  c->owned.push_back(mem);
  p = (T *) mem;
  return hipSuccess;
}
template <class T>
int dev_alloc(pb_ctx *c, T *&p, size_t count)
{
  hipError_t e = dev_alloc_hip(c, p, count);
  return e == hipSuccess ? PB_OK : fail(c, PB_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
}
// a buffer that is re-made: freed and forgotten, p = NULL (the caller has made sure that nothing in flight still uses it).  Only what
// the context owns is freed: a pointer that dev_alloc did not record is dropped, not passed to the runtime.
template <class T>
hipError_t dev_release(pb_ctx *c, T *&p)
{
  const auto at = std::find(c->owned.begin(), c->owned.end(), (void *) p);
  p = nullptr;
  if (at == c->owned.end()) return hipSuccess;
  void *mem = *at;
  c->owned.erase(at);
  return hipFree(mem);
}

// checkpoint slot `slot` of pb_history_reserve
inline double *slot_ptr(const pb_ctx *c, int slot) { return c->hist + (size_t) slot * c->state_doubles; }

// Where an update writes its posterior.  Normally in place.  With pb_set_output_slot the posterior goes straight into a
// checkpoint slot (a checkpoint per update without a copy: the step moves the same bytes either way).  If the head IS a
// checkpoint slot and no output slot was named, the update writes back into the context's own array, so a saved
// posterior is never modified.
int detach_head(pb_ctx *c, bool keep_contents);

inline double *update_target(pb_ctx *c)
{
  if (c->out_slot >= 0) return slot_ptr(c, c->out_slot);
  return (c->st != c->st_base) ? c->st_base : c->st;
}
inline void update_done(pb_ctx *c, double *target)
{
  c->st = target;
  c->out_slot = -1;
}

#define LAUNCHCHK(c) HIPCHK((c), hipGetLastError())

// the cache policy of the state round trip (MemHint; Policy::mem_hint) as a compile-time constant: f(MH)
template <class F>
static void with_mem_hint(int mem_hint, F f)
{
  switch (mem_hint) {
  case MH_STORE_SC1: f(std::integral_constant<int, MH_STORE_SC1>()); break;
  case MH_STREAM_NT: f(std::integral_constant<int, MH_STREAM_NT>()); break;
  default: f(std::integral_constant<int, MH_DEFAULT>()); break;
  }
}
// the state size as a compile-time constant: f(NS), for the launches that differ in nothing else
template <class F>
static void with_ns(int ns, F f)
{
  if (ns == 15) f(std::integral_constant<int, 15>());
  else f(std::integral_constant<int, 21>());
}

// staging area for PB_HOST inputs/outputs (pronto_batch.hip): a device buffer of at least `bytes`
int stage_reserve(pb_ctx *c, size_t bytes);
// Resolve the caller buffers of one call (up to 7: pb_step_legodo_correct): device pointers pass through; host buffers are packed into the staging area.
struct Part {
  const void *src;
  size_t bytes;
  const void *dev;
};
int stage_in(pb_ctx *c, int mem, Part *parts, int n);
// The IMU block of a call, resolved into p[0] (with the n - 1 parts behind it that live in the same space) or, PB_HOST_BROADCAST, into
// bc (pronto_batch.hip)
int imu_in(pb_ctx *c, const double *imu_block, int imu_mem, StepBcast &bc, Part *p, int n = 1);
// the joint-state inputs of one message as the kernels take them (LegIn kind 1; pb_legodo.hip)
int leg_in_joints(pb_ctx *c, const char *who, int n_rows, const float *jpos, const float *jeff, const float *forces, int mem, LegIn &in);
// the frame of a timed entry point: device time between the two events (elapsed_ms NULL: not timed, no event)
int timed_begin(pb_ctx *c, const float *elapsed_ms);
int timed_end(pb_ctx *c, float *elapsed_ms);

// Small read-back of one filter's handler state: `launch(dp, di)` leaves up to 16 doubles and 4 info words in the staging area
template <class Launch>
static int get_small(pb_ctx *c, double *d_out, int n_d, int64_t info[4], Launch launch)
{
  int rc = stage_reserve(c, 256);
  if (rc) return rc;
  double *dp = (double *) c->stage;
  int64_t *di = (int64_t *) (dp + 16);
  rc = launch(dp, di);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(d_out, dp, sizeof(double) * n_d, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, di, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

// ---- the per-call contract: what an entry point takes from the context, declared in ONE line at its top -- CALL(c, flags) ----
// The one-shot inputs belong to the NEXT call that takes them, whatever becomes of it: the pb_set_imu_valid mask to the next call that
// takes an IMU step, the per-filter message times / validity (pb_legodo_set_message_times) to the next odometry or pair call,
// pb_set_pred_slot to the next pb_step_legodo / pb_step_legodo_split / pb_step_legodo_correct.  The guard takes them FIRST, before anything is validated, so
// that a call that fails early cannot leave them behind for an unrelated later call, and forgets them when the call returns.
enum : unsigned {
  IMU_STEP = 1,      // takes the IMU validity mask: held in imu_valid_cur for the duration of the call (pbk_idle_prepare)
  LEG_TIMES = 2,     // takes the message times / validity (Call::times)
  PRED_TAKE = 4,     // writes a predicted posterior: consumes a pending predicted slot, whatever becomes of the call
  PRED_REFUSE = 8,   // takes an IMU step or an update but writes no predicted posterior: with a slot pending it refuses and forgets it
  PRED_FORGET = 16,  // runs a whole log of steps with predicted slots of its own: a pending one is forgotten
  NEEDS_STATE = 32,  // PB_ERR_STATE before pb_reset
  PRED_WITH_OUT = 64,  // (with PRED_TAKE) a checkpointed step only: a predicted slot without a pending output slot is refused as by PRED_REFUSE
};
struct LegMsgTimes {
  const int64_t *utimes = nullptr;
  const uint8_t *valid = nullptr;
};
struct Call {
  pb_ctx *const c;
  const unsigned what;
  LegMsgTimes times;
  int rc;
  Call(pb_ctx *ctx, const char *fn, unsigned flags) : c(ctx), what(flags) { rc = enter(fn); }
  Call(const Call &) = delete;
  ~Call()
  {
    if (!c) return;
    if (what & IMU_STEP) c->imu_valid_cur = c->imu_idle_cur = nullptr;
    if (what & PRED_TAKE) c->pred_slot = -1;
  }

 private:
  int enter(const char *fn)
  {
    if (!c) return PB_ERR_ARG;
    if (what & IMU_STEP) {
      c->imu_valid_cur = c->imu_valid_next;
      c->imu_valid_next = nullptr;
    }
    if (what & LEG_TIMES) {
      if (c->leg_ut_on) times.utimes = c->leg_ut_ext ? c->leg_ut_ext : c->leg_ut;
      if (c->leg_valid_on) times.valid = c->leg_valid_ext ? c->leg_valid_ext : c->leg_valid;
      c->leg_ut_on = c->leg_valid_on = false;
      c->leg_ut_ext = nullptr;
      c->leg_valid_ext = nullptr;
    }
    HIPCHK(c, hipSetDevice(c->dev));
    if ((what & (PRED_REFUSE | PRED_FORGET)) && c->pred_slot >= 0) {
      c->pred_slot = -1;
      if (what & PRED_REFUSE)
        return fail(c, PB_ERR_STATE, "%s: no predicted slot here (pb_set_pred_slot is for pb_step_legodo / _split / _correct)", fn);
    }
    if ((what & PRED_WITH_OUT) && c->pred_slot >= 0 && c->out_slot < 0) {
      c->pred_slot = -1;
      return fail(c, PB_ERR_STATE, "%s: no predicted slot here without an output slot (pb_set_output_slot)", fn);
    }
    if ((what & NEEDS_STATE) && !c->have_state) return fail(c, PB_ERR_STATE, "%s before pb_reset", fn);
    // the pending predicted slot against the slots this call writes / reads (pb_set_output_slot may have come after pb_set_pred_slot)
    if ((what & PRED_TAKE) && c->pred_slot >= 0 && (c->pred_slot >= c->nhist || c->pred_slot == c->out_slot || c->pred_slot == pb_head_slot(c)))
      return fail(c, PB_ERR_ARG, "predicted slot %d: out of range, the output slot or the head's slot", c->pred_slot);
    return PB_OK;
  }
};
#define CALL(c, flags)               \
  Call call((c), __func__, (flags)); \
  if (call.rc) return call.rc

// in front of the ONE step launch of a call that was given a mask (pb_set_imu_valid): the IMU block with the samples of the filters
// WITHOUT a message replaced by what reproduces their angular-velocity / acceleration entries (pb_frontend.hip); the block itself
// when there is no mask.  bc: the call's own copy of its broadcast inputs -- a broadcast IMU sample under a mask becomes a prepared
// block as well, and bc's IMU bit is cleared so that the step reads it
const double *pbk_idle_prepare(pb_ctx *c, const double *imu_dev, StepBcast &bc, int *rc_out);
// behind every step launch of such a call: the process step overwrites the omega and acceleration diagonal blocks of the covariance
// with q_gyro I, q_accel I whatever dt (rbis.cpp:120-121), which the reference did not do for a filter without a message -- they are
// put back (out: the posterior; pred: the predicted slot written by the same launch, or NULL).  Nothing without a mask.
int pbk_idle_restore(pb_ctx *c, double *out, double *pred, const double q[4]);

// ---- launchers defined in the other translation units ----
// pb_step.hip: predict (update = false) or predict + leg-odometry update on the kernel pb_create picked
int pbk_step(pb_ctx *c, bool update, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
             const StepBcast *bcast = nullptr);  // bcast: one message for every filter, as kernel arguments
// the fused step on the filters [b0, b0 + nb) only (whole tiles, in place; pb_run_legodo's cache-blocked order)
int pbk_step_range(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], long b0, int nb, Mapping map, int mem_hint);
// IMU step + leg odometry (from `lin`) + its lin_rate update in ONE kernel; -1 = this context has no such kernel (run
// pb_legodo_update* ahead of pbk_step instead)
// mp.mode 1 / 2: LegOdoCommon's six-row measurements instead (lo_out [12][B], mask_out [2][B] as pb_legodo_set_measurement_mode)
int pbk_step_leg(pb_ctx *c, const double *imu, const StepBcast *bcast, const double q[4], const LegIn &lin, int64_t utime, const LegMeasPar &mp,
                 double *lo_out, uint8_t *mask_out);
// pb_step_leg.hip, one object per state size: the pair kernels' launchers
int pbk_step_leg15(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la);
int pbk_step_leg21(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la);
// pb_legpar.hip, one object per state size: their siblings that read the context's per-filter parameter block (c->leg_blk)
int pbk_legpar15(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la);
int pbk_legpar21(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la);
// slot0 >= 0: write-through -- the posterior of step t also goes to checkpoint slot slot0 + t (pb_replay_legodo_checkpointed)
int pbk_replay_fused(pb_ctx *c, int T, const double *imu, const double *lo, const uint8_t *mask, const double q[4], int slot0 = -1);
// pb_step_pred.hip: the fused step that also writes its predicted posterior into `pred` (k_step_coop_pred); -1 = this context has no
// such kernel (pbk_step then runs the predict into `pred` and the fused step as two launches)
int pbk_step_pred_kernel(pb_ctx *c, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                         const StepBcast &bc);
// pb_step_corr_pred.hip: the 15-state fused step with a correction stage that also writes its predicted posterior into `pred`
// (k_step_coop_corr_pred); -1 = not a 15-state context
int pbk_step_corr_pred_kernel(pb_ctx *c, int corr_kind, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask,
                              const double q[4], const CorrArgs &ca, const StepBcast &bc);
// predict + leg-odometry update + a second (orientation) update in one state round trip; corr_kind = enum pb_corr.  A pending predicted
// slot (c->pred_slot) is consumed: the INS posterior goes there as well
int pbk_step_correct(pb_ctx *c, int corr_kind, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                     const double *z2, const double *r2, const double *rb2, const double *qm2, const uint8_t *mask2,
                     const StepBcast *bcast = nullptr, const double *zb = nullptr, const double *qb = nullptr);
// The inputs of a stand-alone indexed (+ orientation) update as the kernels take them: device blocks [rows][B], or host values that
// travel as kernel arguments.  Exactly one of r_diag / r_bcast / r_full is set.
struct UpdateIn {
  const double *z = nullptr;        // [m][B]
  const double *r_diag = nullptr;   // per-filter R diagonal [m][B]
  const double *r_bcast = nullptr;  // one R diagonal for every filter: m HOST values
  const double *r_full = nullptr;   // per-filter full R [m*m][B], column-major
  const double *qm = nullptr;       // measured quaternion [4][B]
  const uint8_t *mask = nullptr;    // [B] or NULL
  const double *z_host = nullptr;   // UpdateChoice::host_args: z (m HOST values) ...
  const double *q_host = nullptr;   // ... and the measured quaternion (4) of ONE measurement for every filter
  int rkind() const { return r_full ? PB_R_FULL : r_bcast ? PB_R_DIAG_BROADCAST : PB_R_DIAG; }
  const double *R() const { return r_full ? r_full : r_diag; }
};
// pb_update_ct.hip: THE entry to the update kernels -- launches what update_choice (pb_policy.hpp) answered; honours pb_set_output_slot
int pbk_update(pb_ctx *c, const UpdateChoice &u, int m, const int *idx, const UpdateIn &in);
// the run-time-index families and the 21-state list kernel, in the objects that hold them: pb_update.hip (15 states) and
// pb_update_rt21.hip (built as three objects, by m)
int pbk_update15(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in);
int pbk_update21_m123(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in);
int pbk_update21_m45(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in);
int pbk_update21_m6(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in);
// pb_update_wide.hip: family UPD_WIDE, m = 7 ... 9 (k_update_wide, rbis_update_wide.hpp)
int pbk_update_wide(pb_ctx *c, int m, const int *idx, const UpdateIn &in);
// pb_smooth.hip
int pbk_smooth_step(pb_ctx *c, const double *next_pred, const double *next_sm, const double *cur, double *out, double dt);
int pbk_smooth_wide(pb_ctx *c, const double *next_pred, const double *next_sm, const double *cur, double *out, double dt);   // 15 states (pb_smooth_wide.hip)
// pb_select.hip: dst <- src for the filters whose mask_dev entry (device, [B]; non-zero counts as 1) equals `when`, every other column untouched
int pbk_slot_select(pb_ctx *c, double *dst, const double *src, const uint8_t *mask_dev, int when);
// pronto_batch.hip: the stand-alone indexed (+ orientation, orient) update of pb_update_indexed*, on the kernel the index list and R allow;
// honours pb_set_output_slot
int pbk_update_common(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int rkind, const double *qm, bool orient,
                      const uint8_t *mask, int mem);
// its check of an index list: every index inside the state, no index twice
int pbk_check_indices(pb_ctx *c, int m, const int *idx);
