// pb_step_pred.hip -- the fused step that also keeps its prediction (pb_set_pred_slot): k_step_coop_pred / k_step_quad_pred, one object of its own so
// that the step kernels' object (pb_step.hip) stays what it was.
#include "pb_ctx.hpp"
#include "rbis_step_kernels.hpp"

template <int MH>
static int launch_pred_mh(pb_ctx *c, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                          const StepBcast &bc)
{
  const int B = c->B;
  const StepChoice step = c->policy.step;
  switch (step.map) {
  case MAP_COOP15: {
    Consts kk = c->k;
    kk.half_tiles = step.half ? 1 : 0;   // (as launch_step_kernel: this launch only)
    k_step_coop_pred<15, MH><<<nblk(B) * (step.half ? 2 : 1), 128, 0, c->stream>>>(c->st, out, pred, B, imu, lo, mask, q[0], q[1], q[2], q[3], kk, bc);
    return PB_OK;
  }
  case MAP_QUAD21:
    k_step_quad_pred<MH><<<nblk(B), 256, 0, c->stream>>>(c->st, out, pred, B, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, bc);
    return PB_OK;
  case MAP_COOP21:
    k_step_coop_pred<21, MH><<<nblk(B), 128, 0, c->stream>>>(c->st, out, pred, B, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, bc);
    return PB_OK;
  default:  // MAP_LANE15: pred_kernel_exists() is false, the caller runs two launches
    return -1;
  }
}

int pbk_step_pred_kernel(pb_ctx *c, double *out, double *pred, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                         const StepBcast &bc)
{
  int rc = -1;
  if (!pred_kernel_exists(c->policy.step.map)) return rc;
  with_mem_hint(c->policy.mem_hint, [&](auto mh) { rc = launch_pred_mh<decltype(mh)::value>(c, out, pred, imu, lo, mask, q, bc); });
  return rc;
}
