// pb_step_corr_pred.hip -- the 15-state fused step with a correction stage that also keeps its prediction (pb_set_pred_slot in front of
// pb_step_legodo_correct): k_step_coop_corr_pred, one object of its own so that the step kernels' objects (pb_step.hip,
// pb_step_pred.hip) stay what they were.
#include "pb_ctx.hpp"
#include "rbis_step_kernels.hpp"

template <int MH, class CORR>
static void launch_corr_pred(pb_ctx *c, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                             const CorrArgs &ca, const StepBcast &bc)
{
  k_step_coop_corr_pred<15, MH, CORR><<<nblk(c->B), 128, 0, c->stream>>>(c->st, out, pred, c->B, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, ca, bc);
}

template <int MH>
static int launch_corr_pred_mh(pb_ctx *c, int corr_kind, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask,
                               const double q[4], const CorrArgs &ca, const StepBcast &bc)
{
  if (c->ns != 15) return -1;
  if (corr_kind == PB_CORR_POS_ORIENT) launch_corr_pred<MH, CorrPosOrient>(c, out, pred, imu, lo, mask, q, ca, bc);
  else launch_corr_pred<MH, CorrPosYaw>(c, out, pred, imu, lo, mask, q, ca, bc);
  return PB_OK;
}

int pbk_step_corr_pred_kernel(pb_ctx *c, int corr_kind, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask,
                              const double q[4], const CorrArgs &ca, const StepBcast &bc)
{
  int rc = -1;
  with_mem_hint(c->policy.mem_hint, [&](auto mh) { rc = launch_corr_pred_mh<decltype(mh)::value>(c, corr_kind, out, pred, imu, lo, mask, q, ca, bc); });
  return rc;
}
