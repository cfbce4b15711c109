// pb_legpar.hip -- launchers of the pair kernels that read the leg odometry's noises and contact thresholds per filter
// (rbis_legstep.hpp k_pair_legpar / k_pair_quad_legpar, rbis_legpar.hpp; pb_legodo_set_param_block): the siblings of pb_step_leg.hip's
// kernels, in objects of their own.  Built as two objects (-DPB_LEG_NS=15 | 21), each with the three measurement modes x the three
// cache policies.
#include "pb_ctx.hpp"
#include "rbis_legstep.hpp"

#ifndef PB_LEG_NS
#error "PB_LEG_NS = 15 | 21"
#endif

template <int SIX>
static void launch_legpar(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin,
                          const LegStepArgs &la)
{
  const LegParRows rows{ c->leg_blk, c->stride };
  with_mem_hint(c->policy.mem_hint, [&](auto mh) {
    constexpr int MH = decltype(mh)::value;
#define LEG_ARGS c->st, out, c->B, imu, q[0], q[1], q[2], q[3], c->k, bc, c->leg_par, lin, c->leg_chain, la, rows
#if PB_LEG_NS == 15
    k_pair_legpar<15, MH, SIX><<<nblk(c->B), 128, 0, c->stream>>>(LEG_ARGS);
#else
    k_pair_quad_legpar<MH, SIX><<<nblk(c->B), 256, 0, c->stream>>>(LEG_ARGS);
#endif
#undef LEG_ARGS
  });
}

#if PB_LEG_NS == 15
int pbk_legpar15(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la)
#else
int pbk_legpar21(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la)
#endif
{
  switch (la.mp.mode) {
  case 1: launch_legpar<1>(c, out, imu, q, bc, lin, la); break;
  case 2: launch_legpar<2>(c, out, imu, q, bc, lin, la); break;
  default: launch_legpar<0>(c, out, imu, q, bc, lin, la); break;
  }
  return PB_OK;
}
