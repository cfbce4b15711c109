// pb_history.hip -- the checkpoint slots (pb_history_reserve), where the head and the next posteriors live among them, the per-filter
// selection between posteriors, and RTS smoothing over the slots: single steps and whole logs.  No kernel is defined or included
// here: everything is launched through the pbk_* launchers of the other units.  See pb_ctx.hpp.
#include "pb_ctx.hpp"

// the head goes back to the context's own array (copying it there if it currently lives in a checkpoint slot)
int detach_head(pb_ctx *c, bool keep_contents)
{
  if (c->st != c->st_base) {
    if (keep_contents)
      HIPCHK(c, hipMemcpyAsync(c->st_base, c->st, sizeof(double) * c->state_doubles, hipMemcpyDeviceToDevice, c->stream));
    c->st = c->st_base;
  }
  c->out_slot = -1;
  return PB_OK;
}

extern "C" int pb_history_reserve(pb_ctx *c, int n_slots)
{
  CALL(c, 0);
  if (n_slots < 0) return fail(c, PB_ERR_ARG, "pb_history_reserve: n_slots < 0");
  int rc = detach_head(c, true);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->nhist = 0;
  c->pred_slot = -1;
  HIPCHK(c, dev_release(c, c->hist));
  if (n_slots == 0) return PB_OK;
  const size_t bytes = sizeof(double) * c->state_doubles;
  hipError_t e = dev_alloc_hip(c, c->hist, c->state_doubles * n_slots);
  if (e != hipSuccess)
    return fail(c, PB_ERR_HIP, "pb_history_reserve: %d slots x %zu bytes: %s", n_slots, bytes, hipGetErrorString(e));
  // the padding columns (batch rounded up to 64) of a slot are read by the cooperative kernel's idle lanes
  HIPCHK(c, hipMemsetAsync(c->hist, 0, bytes * n_slots, c->stream));
  c->nhist = n_slots;
  return PB_OK;
}

extern "C" int pb_set_output_slot(pb_ctx *c, int slot)
{
  CALL(c, 0);
  if (slot < -1 || slot >= c->nhist) return fail(c, PB_ERR_STATE, "pb_set_output_slot: checkpoint slot %d of %d", slot, c->nhist);
  c->out_slot = slot;
  return PB_OK;
}

extern "C" int pb_set_pred_slot(pb_ctx *c, int slot)
{
  CALL(c, 0);
  if (slot == -1) {
    c->pred_slot = -1;
    return PB_OK;
  }
  if (slot < 0 || slot >= c->nhist) return fail(c, PB_ERR_ARG, "pb_set_pred_slot: checkpoint slot %d of %d", slot, c->nhist);
  if (slot == c->out_slot) return fail(c, PB_ERR_ARG, "pb_set_pred_slot: slot %d is the pending output slot", slot);
  if (slot == pb_head_slot(c)) return fail(c, PB_ERR_ARG, "pb_set_pred_slot: slot %d holds the head", slot);
  c->pred_slot = slot;
  return PB_OK;
}

extern "C" int pb_head_slot(const pb_ctx *c)
{
  if (!c || c->st == c->st_base || !c->hist) return -1;
  return (int) ((size_t) (c->st - c->hist) / c->state_doubles);
}

extern "C" int pb_state_save(pb_ctx *c, int slot)
{
  CALL(c, NEEDS_STATE);
  if (slot < 0 || slot >= c->nhist) return fail(c, PB_ERR_STATE, "checkpoint slot %d of %d", slot, c->nhist);
  const size_t n = c->state_doubles;
  double *h = slot_ptr(c, slot);
  if (h == c->st) return PB_OK;  // the head was written straight into this slot (pb_set_output_slot)
  HIPCHK(c, hipMemcpyAsync(h, c->st, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  return PB_OK;
}

extern "C" int pb_state_restore(pb_ctx *c, int slot)
{
  CALL(c, NEEDS_STATE);
  if (slot < 0 || slot >= c->nhist) return fail(c, PB_ERR_STATE, "checkpoint slot %d of %d", slot, c->nhist);
  const size_t n = c->state_doubles;
  // always into the context's own array: the slot the head may currently live in stays what it is
  HIPCHK(c, hipMemcpyAsync(c->st_base, slot_ptr(c, slot), sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  c->st = c->st_base;
  c->out_slot = -1;
  return PB_OK;
}

extern "C" int pb_smooth_step(pb_ctx *c, int slot_next_pred, int slot_next, int slot_cur, int slot_out, double dt)
{
  CALL(c, 0);
  const int s[4] = { slot_next_pred, slot_next, slot_cur, slot_out };
  for (int i = 0; i < 4; i++)
    if (s[i] < 0 || s[i] >= c->nhist) return fail(c, PB_ERR_STATE, "pb_smooth_step: checkpoint slot %d of %d", s[i], c->nhist);
  if (slot_out == slot_next_pred || slot_out == slot_next)
    return fail(c, PB_ERR_ARG, "pb_smooth_step: slot_out may alias slot_cur only");
  return pbk_smooth_step(c, slot_ptr(c, slot_next_pred), slot_ptr(c, slot_next), slot_ptr(c, slot_cur), slot_ptr(c, slot_out), dt);
}

// ---- per-filter selection between posteriors (independent log segments of different lengths) ----
extern "C" int pb_slot_select(pb_ctx *c, int dst, int src, const uint8_t *mask, int when, int mem)
{
  CALL(c, 0);
  for (int sl : { dst, src })
    if (sl < PB_SLOT_HEAD || sl >= c->nhist) return fail(c, PB_ERR_STATE, "pb_slot_select: checkpoint slot %d of %d", sl, c->nhist);
  if (!mask) return fail(c, PB_ERR_ARG, "pb_slot_select: NULL mask");
  if (when != 0 && when != 1) return fail(c, PB_ERR_ARG, "pb_slot_select: when = %d (0 or 1)", when);
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_slot_select: mem must be PB_HOST or PB_DEVICE");
  if ((dst == PB_SLOT_HEAD || src == PB_SLOT_HEAD) && !c->have_state) return fail(c, PB_ERR_STATE, "pb_slot_select: the head before pb_reset");
  double *d = dst == PB_SLOT_HEAD ? c->st : slot_ptr(c, dst);
  const double *s = src == PB_SLOT_HEAD ? c->st : slot_ptr(c, src);
  if (d == s) return PB_OK;
  Part p[1] = { { mask, (size_t) c->B, 0 } };
  int rc = stage_in(c, mem, p, 1);
  if (rc) return rc;
  return pbk_slot_select(c, d, s, (const uint8_t *) p[0].dev, when);
}

extern "C" int pb_smooth_step_masked(pb_ctx *c, int slot_next_pred, int slot_next, int slot_cur, int slot_out, double dt, const uint8_t *step,
                                     int mem)
{
  if (int rc = pb_smooth_step(c, slot_next_pred, slot_next, slot_cur, slot_out, dt)) return rc;
  if (!step) return PB_OK;
  return pb_slot_select(c, slot_out, slot_next, step, 0, mem);   // (slot_out != slot_next: pb_smooth_step checked it)
}

// ---- whole-log RTS smoothing with bounded memory: checkpoint and recompute ----
// EKFSmoothBackwardsPass (mav_state_est.cpp:98-189) walks the WHOLE history backwards and reads, at every INS update, three
// posteriors the reference keeps by value in its update objects.  For a batch that is 2 T slots of the whole state (64k 21-state
// filters: 135 MB each -- one second of a 1 kHz log fills 288 GB).  Here the forward pass keeps only every `stride`-th posterior;
// the backward pass takes the log stretch by stretch, newest first: it re-runs the stretch's steps from its checkpoint into a
// window of 2 * stride slots (the posterior of every process step AND of the update behind it, with the very kernels the
// per-message path runs: pb_predict, pb_update_indexed) and smooths it with the smoother step.  Slots: T / stride + 2 stride + 4.
extern "C" int pb_smooth_log_slots(int n_steps, int stride)
{
  if (n_steps < 1 || stride < 1) return -1;
  return (n_steps + stride - 1) / stride + 2 * stride + 4;
}

// fused: every step of the forward pass and of the recompute pass is ONE launch with the semantics of pb_step_legodo, which in the
// recompute pass writes the window's predicted slot (pb_set_pred_slot) and its filtered slot together; otherwise the process step and
// LegOdoCommon's lin_rate update exactly as the per-message path applies them (pb_predict, pb_update_indexed).  Same slots, sink order
// and head afterwards.  On an error the head goes back to the context's own array (the pre-call head, or the newest posterior once
// the forward pass is over) and no output / predicted slot is left pending.
// corr (pb_smooth_log_corrected; NULL or no ticks: none): a step with a tick takes the tick's correction behind its pair, in both
// passes -- fused as pb_step_legodo_correct does (pbk_step_correct, which also takes the predicted slot), otherwise as one more
// pb_update_indexed_orient into the step's filtered slot.  "Filtered" is then the posterior of the step's LAST measurement.
static int smooth_log_impl(pb_ctx *c, const char *who, bool fused, int n_steps, int stride, const double *imu_stream, const double *lo_stream,
                           const uint8_t *mask_stream, const double q[4], double dt, int first_slot, pb_smooth_sink sink, void *user, float *elapsed_ms,
                           const pb_corr_stream *corr = nullptr)
{
  if (n_steps < 1 || stride < 1 || !imu_stream || !lo_stream || !q) return fail(c, PB_ERR_ARG, "%s: bad argument", who);
  const int n_ticks = corr ? corr->n_ticks : 0;
  int m2 = 0, r_kind2 = PB_R_DIAG;
  const int *idx2 = nullptr;
  if (n_ticks != 0) {
    static const int idx_po[6] = { 9, 10, 11, 6, 7, 8 }, idx_py[4] = { 9, 10, 11, 8 };
    if (corr->kind != PB_CORR_POS_ORIENT && corr->kind != PB_CORR_POS_YAW) return fail(c, PB_ERR_ARG, "%s: bad correction kind %d", who, corr->kind);
    m2 = (corr->kind == PB_CORR_POS_ORIENT) ? 6 : 4;
    idx2 = (corr->kind == PB_CORR_POS_ORIENT) ? idx_po : idx_py;
    r_kind2 = corr->r_kind2;
    if (n_ticks < 0 || !corr->step || !corr->z2 || !corr->R2 || !corr->quat_meas2) return fail(c, PB_ERR_ARG, "%s: correction stream: NULL input", who);
    if (r_kind2 != PB_R_DIAG && r_kind2 != PB_R_DIAG_BROADCAST) return fail(c, PB_ERR_ARG, "%s: R2 must be diagonal (PB_R_DIAG or PB_R_DIAG_BROADCAST)", who);
    for (int t = 0; t < n_ticks; t++)
      if (corr->step[t] < 0 || corr->step[t] >= n_steps || (t > 0 && corr->step[t] <= corr->step[t - 1]))
        return fail(c, PB_ERR_ARG, "%s: correction steps must be strictly increasing and in [0, %d) (entry %d: %d)", who, n_steps, t, corr->step[t]);
  }
  const int K = stride, T = n_steps, M = (T + K - 1) / K, need = pb_smooth_log_slots(T, K);
  if (first_slot < 0 || first_slot + need > c->nhist)
    return fail(c, PB_ERR_STATE, "%s: needs checkpoint slots [%d, %d), %d are reserved (pb_history_reserve)", who, first_slot, first_slot + need, c->nhist);
  const size_t B = (size_t) c->B, n = c->state_doubles;
  const int CK = first_slot, WP = CK + M, WF = WP + K, PC = WF + K, FIN = PC + 1, SP = FIN + 1;   // checkpoints | window | carry | final | ping-pong
  bool have_fin = false;
  auto bail = [&](int code) -> int {
    c->out_slot = -1;
    c->pred_slot = -1;
    if (c->st != c->st_base) {   // (backward pass: the head lives in a checkpoint or window slot)
      if (have_fin) (void) hipMemcpyAsync(c->st_base, slot_ptr(c, FIN), sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream);
      c->st = c->st_base;
    }
    return code;
  };
  static const int idx_v[3] = { 3, 4, 5 };
  // one step of the log (pred_slot / filt_slot < 0: in place)
  auto step = [&](int j, int pred_slot, int filt_slot) -> int {
    const double *imu = imu_stream + (size_t) j * 7 * B, *lo = lo_stream + (size_t) j * 6 * B;
    const uint8_t *mask = mask_stream ? mask_stream + (size_t) j * B : nullptr;
    // this step's correction tick, if it has one
    const double *z2 = nullptr, *R2 = nullptr, *qm2 = nullptr;
    const uint8_t *mask2 = nullptr;
    if (n_ticks > 0) {
      const int32_t *at = std::lower_bound(corr->step, corr->step + n_ticks, (int32_t) j);
      if (at != corr->step + n_ticks && *at == j) {
        const size_t t = (size_t) (at - corr->step);
        z2 = corr->z2 + t * m2 * B;
        R2 = (r_kind2 == PB_R_DIAG) ? corr->R2 + t * m2 * B : corr->R2;
        qm2 = corr->quat_meas2 + t * 4 * B;
        mask2 = corr->mask2 ? corr->mask2 + t * B : nullptr;
      }
    }
    if (fused) {
      c->pred_slot = pred_slot;
      c->out_slot = filt_slot;
      const int r = z2 ? pbk_step_correct(c, corr->kind, imu, lo, mask, q, z2, r_kind2 == PB_R_DIAG ? R2 : nullptr,
                                          r_kind2 == PB_R_DIAG ? nullptr : R2, qm2, mask2)
                       : pbk_step(c, true, imu, lo, mask, q);
      c->pred_slot = -1;
      return r;
    }
    c->out_slot = pred_slot;
    int rc = pbk_step(c, false, imu, nullptr, nullptr, q);
    if (rc) return rc;
    c->out_slot = filt_slot;
    rc = pbk_update_common(c, 3, idx_v, lo, lo + 3 * B, PB_R_DIAG, nullptr, false, mask, PB_DEVICE);
    if (rc || !z2) return rc;
    c->out_slot = filt_slot;   // the correction lands where the pair's posterior is
    return pbk_update_common(c, m2, idx2, z2, R2, r_kind2, qm2, true, mask2, PB_DEVICE);
  };
  int rc = timed_begin(c, elapsed_ms);
  if (rc || (rc = detach_head(c, true))) return bail(rc);
  // ---- forward: the filter, a checkpoint in front of every stretch ----
  for (int j = 0; j < T; j++) {
    if (j % K == 0 && (rc = pb_state_save(c, CK + j / K))) return bail(rc);
    if ((rc = step(j, -1, -1))) return bail(rc);
  }
  if ((rc = pb_state_save(c, FIN))) return bail(rc);   // the newest posterior: its own smoothed value (and the head again when the pass is over)
  have_fin = true;
  // ---- backward: stretch by stretch ----
  int next_sm = FIN, toggle = 0;
  for (int m = M - 1; m >= 0; m--) {
    const int s0 = m * K, s1 = std::min(T, s0 + K) - 1;
    c->st = slot_ptr(c, CK + m);   // the head lives in the checkpoint: the first process step reads it there and writes into the window
    c->out_slot = -1;
    for (int j = s0; j <= s1; j++)
      if ((rc = step(j, WP + (j - s0), WF + (j - s0)))) return bail(rc);
    for (int j = s1; j >= s0; j--) {
      if (j == T - 1) continue;   // (the newest step is not smoothed: mav_state_est.cpp:120-131 starts one step behind it)
      const int np = (j == s1) ? PC : WP + (j + 1 - s0);
      const int out = SP + toggle;
      if ((rc = pbk_smooth_step(c, slot_ptr(c, np), slot_ptr(c, next_sm), slot_ptr(c, WF + (j - s0)), slot_ptr(c, out), dt))) return bail(rc);
      if (sink) sink(user, j, out);
      next_sm = out;
      toggle ^= 1;
    }
    // the earlier stretch's last step needs the process-step posterior of THIS stretch's first step
    if (hipMemcpyAsync(slot_ptr(c, PC), slot_ptr(c, WP), sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
      return bail(fail(c, PB_ERR_HIP, "%s: carry copy", who));
  }
  if ((rc = pb_state_restore(c, FIN))) return bail(rc);
  return timed_end(c, elapsed_ms);
}

extern "C" int pb_smooth_log(pb_ctx *c, int n_steps, int stride, const double *imu_stream, const double *lo_stream, const uint8_t *mask_stream,
                             const double q[4], double dt, int first_slot, pb_smooth_sink sink, void *user, float *elapsed_ms)
{
  CALL(c, PRED_FORGET | NEEDS_STATE);
  return smooth_log_impl(c, "pb_smooth_log", false, n_steps, stride, imu_stream, lo_stream, mask_stream, q, dt, first_slot, sink, user, elapsed_ms);
}

extern "C" int pb_smooth_log_fused(pb_ctx *c, int n_steps, int stride, const double *imu_stream, const double *lo_stream,
                                   const uint8_t *mask_stream, const double q[4], double dt, int first_slot, pb_smooth_sink sink,
                                   void *user, float *elapsed_ms)
{
  CALL(c, PRED_FORGET | NEEDS_STATE);
  // (ahead of the argument checks: also a call that is refused for its arguments or slots leaves the head in the context's own array)
  if (int rc = detach_head(c, true)) return rc;
  return smooth_log_impl(c, "pb_smooth_log_fused", true, n_steps, stride, imu_stream, lo_stream, mask_stream, q, dt, first_slot, sink, user, elapsed_ms);
}

extern "C" int pb_smooth_log_corrected(pb_ctx *c, int n_steps, int stride, const double *imu_stream, const double *lo_stream,
                                       const uint8_t *mask_stream, const double q[4], double dt, int first_slot, const pb_corr_stream *corr,
                                       int fused, pb_smooth_sink sink, void *user, float *elapsed_ms)
{
  CALL(c, PRED_FORGET | NEEDS_STATE);
  // (ahead of the argument checks, as pb_smooth_log_fused: a refused call too leaves the head in the context's own array)
  if (int rc = detach_head(c, true)) return rc;
  return smooth_log_impl(c, "pb_smooth_log_corrected", fused != 0, n_steps, stride, imu_stream, lo_stream, mask_stream, q, dt, first_slot, sink, user,
                         elapsed_ms, corr);
}
