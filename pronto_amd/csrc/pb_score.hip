// pb_score.hip -- drift per distance travelled against ground truth (rbis_score.hpp): the kernels (rbis_score_kernels.hpp), their
// launches and the pb_score_* entry points of the C ABI.  See pb_ctx.hpp.
//
// Nothing here writes a filter's state or takes one of the context's one-shot inputs: the entry points run under CALL(c, 0 /
// NEEDS_STATE), which leaves a pending pb_set_output_slot / pb_set_pred_slot where it is.
#include "pb_ctx.hpp"
#include "rbis_score_kernels.hpp"

// State.__init__ (drift_per_distance.py:25-40)
extern "C" int pb_score_init(pb_ctx *c, double time_threshold_s, double distance_threshold)
{
  CALL(c, 0);
  if (!(time_threshold_s >= 0.0) || !(distance_threshold >= 0.0))
    return fail(c, PB_ERR_ARG, "pb_score_init: thresholds must be >= 0 (time %g s, distance %g m)", time_threshold_s, distance_threshold);
  if (int rc = dev_alloc(c, c->scored, PB_SCORE_ROWS * (size_t) c->stride)) return rc;
  if (int rc = dev_alloc(c, c->scorei, PB_SCORE_COUNTS * (size_t) c->stride)) return rc;
  c->score_par.time_threshold_s = time_threshold_s;
  c->score_par.distance_threshold = distance_threshold;
  k_score_reset<<<nblk((int) c->stride), 64, 0, c->stream>>>(c->scored, c->scorei, c->stride);
  LAUNCHCHK(c);
  return PB_OK;
}

// on_pose_gt (drift_per_distance.py:70-138) with most_recent_est (on_pose_est, :53-56) read from the filter state
extern "C" int pb_score_ground_truth(pb_ctx *c, int64_t utime, const int64_t *utimes, const double *pose7, const uint8_t *valid, int slot,
                                     int flags, int mem)
{
  CALL(c, NEEDS_STATE);
  if (!c->scored) return fail(c, PB_ERR_STATE, "pb_score_ground_truth before pb_score_init");
  if (slot < PB_SLOT_HEAD || slot >= c->nhist) return fail(c, PB_ERR_STATE, "pb_score_ground_truth: checkpoint slot %d of %d", slot, c->nhist);
  if (!pose7) return fail(c, PB_ERR_ARG, "pb_score_ground_truth: NULL pose");
  if (flags == 0 || (flags & ~(PB_SCORE_DRIFT | PB_SCORE_ABS))) return fail(c, PB_ERR_ARG, "pb_score_ground_truth: flags = %d (PB_SCORE_DRIFT | PB_SCORE_ABS)", flags);
  if (mem != PB_HOST && mem != PB_DEVICE && mem != PB_HOST_BROADCAST) return fail(c, PB_ERR_ARG, "pb_score_ground_truth: mem must be PB_HOST, PB_DEVICE or PB_HOST_BROADCAST");
  const size_t B = (size_t) c->B;
  ScoreGt gt;
  gt.utime = utime;
  // one robot's truth: the seven values are kernel arguments; the per-filter times / validity, if any, are host arrays
  const bool bcast = mem == PB_HOST_BROADCAST;
  if (bcast) memcpy(gt.bc, pose7, sizeof gt.bc);
  Part p[3] = { { bcast ? nullptr : pose7, bcast ? 0 : sizeof(double) * 7 * B, 0 }, { utimes, utimes ? sizeof(int64_t) * B : 0, 0 },
                { valid, valid ? B : 0, 0 } };
  if (!bcast || utimes || valid) {
    int rc = stage_in(c, bcast ? PB_HOST : mem, p, 3);
    if (rc) return rc;
  }
  gt.pose = (const double *) p[0].dev;
  gt.utimes = (const int64_t *) p[1].dev;
  gt.valid = (const uint8_t *) p[2].dev;
  // the array the estimate is read from: where the head lives now (as pb_slot_select resolves PB_SLOT_HEAD), or a checkpoint slot
  const double *st = slot == PB_SLOT_HEAD ? c->st : slot_ptr(c, slot);
  with_ns(c->ns, [&](auto NS) {
    k_score_gt<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(st, c->B, c->stride, c->score_par, flags, gt, c->scored, c->scorei);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_score_get(pb_ctx *c, int first, int count, double *rows_out, int64_t *counts_out, int mem)
{
  CALL(c, 0);
  if (!c->scored) return fail(c, PB_ERR_STATE, "pb_score_get before pb_score_init");
  if (first < 0 || count < 0 || (long) first + count > c->B) return fail(c, PB_ERR_ARG, "pb_score_get: range [%d,+%d) outside batch %d", first, count, c->B);
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_score_get: mem must be PB_HOST or PB_DEVICE");
  if (count == 0) return PB_OK;
  const hipMemcpyKind kind = mem == PB_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const size_t w = sizeof(double) * (size_t) count, pitch = sizeof(double) * (size_t) c->stride;  // (both element types are 8 bytes)
  if (rows_out) HIPCHK(c, hipMemcpy2DAsync(rows_out, w, c->scored + first, pitch, w, PB_SCORE_ROWS, kind, c->stream));
  if (counts_out) HIPCHK(c, hipMemcpy2DAsync(counts_out, w, c->scorei + first, pitch, w, PB_SCORE_COUNTS, kind, c->stream));
  if (mem == PB_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

// error_metrics_t of the newest window (drift_per_distance.py:124-133)
extern "C" int pb_score_last(pb_ctx *c, int filter, int64_t *utime, double out[10])
{
  CALL(c, 0);
  if (!c->scored) return fail(c, PB_ERR_STATE, "pb_score_last before pb_score_init");
  if (filter < 0 || filter >= c->B || !utime || !out) return fail(c, PB_ERR_ARG, "pb_score_last: bad argument");
  const size_t pitch = sizeof(double) * (size_t) c->stride;
  HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double), c->scored + (size_t) PB_SCORE_LAST_POS_ERROR * c->stride + filter, pitch, sizeof(double), 10,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(utime, c->scorei + (size_t) PB_SCORE_LAST_UTIME * c->stride + filter, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

extern "C" int pb_score_best(pb_ctx *c, int metric, int *filter_out, double *value_out)
{
  CALL(c, 0);
  if (!c->scored) return fail(c, PB_ERR_STATE, "pb_score_best before pb_score_init");
  if (metric != PB_SCORE_MEAN_PDDT && metric != PB_SCORE_RMS_DRIFT && metric != PB_SCORE_ATE_RMSE)
    return fail(c, PB_ERR_ARG, "pb_score_best: metric = %d", metric);
  if (!filter_out) return fail(c, PB_ERR_ARG, "pb_score_best: NULL filter_out");
  const int n_part = (c->B + SCORE_BEST_PER_WG - 1) / SCORE_BEST_PER_WG;
  // staging: [n_part + 1] values, then [n_part + 1] indices (the last of each is the result)
  const size_t off_f = (sizeof(double) * ((size_t) n_part + 1) + 255) / 256 * 256;
  int rc = stage_reserve(c, off_f + sizeof(int) * ((size_t) n_part + 1));
  if (rc) return rc;
  double *pv = (double *) c->stage;
  int *pf = (int *) ((char *) c->stage + off_f);
  k_score_best_part<<<n_part, 64, 0, c->stream>>>(c->scored, c->scorei, c->stride, c->B, metric, pv, pf);
  LAUNCHCHK(c);
  k_score_best_final<<<1, 64, 0, c->stream>>>(pv, pf, n_part, pv + n_part, pf + n_part);
  LAUNCHCHK(c);
  double v = 0.0;
  int f = -1;
  HIPCHK(c, hipMemcpyAsync(&v, pv + n_part, sizeof v, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&f, pf + n_part, sizeof f, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *filter_out = f;
  if (value_out) *value_out = v;
  return PB_OK;
}
