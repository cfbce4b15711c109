// pb_step_leg.hip -- launchers of the pair kernels (rbis_legstep.hpp): IMU step + leg odometry + its update in one kernel.
// Built as two objects (-DPB_LEG_NS=15 | 21: k_step_leg | k_step_quad_leg) so that `make -j` compiles them side by side;
// each holds the three measurement modes (SIX = 0 lin_rate, 1 lin_rot_rate, 2 pos_and_lin_rate) x the three cache policies.
#include "pb_ctx.hpp"
#include "rbis_legstep.hpp"

#ifndef PB_LEG_NS
#error "PB_LEG_NS = 15 | 21"
#endif

template <int MH, int SIX>
static void launch_step_leg(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin,
                            const LegStepArgs &la)
{
  // (the division of the leg work between the waves, PLAN, and the number of panel rows role P requests ahead of the odometry,
  // EARLY, are template parameters of rbis_legstep.hpp; only the measured best is instantiated -- 12 rows in every mode.  The
  // parameters and the other PLAN branches inside the kernels stay: they are part of the kernel names the profiles and tests key on.)
#define LEG_ARGS c->st, out, c->B, imu, q[0], q[1], q[2], q[3], c->k, bc, c->leg_par, lin, c->leg_chain, la
#if PB_LEG_NS == 15
  k_step_leg<15, MH, 0, 12, SIX><<<nblk(c->B), 128, 0, c->stream>>>(LEG_ARGS);
#else
  k_step_quad_leg<MH, 3, 0, SIX><<<nblk(c->B), 256, 0, c->stream>>>(LEG_ARGS);
#endif
#undef LEG_ARGS
}

template <int SIX>
static void launch_step_leg_mh(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin,
                               const LegStepArgs &la)
{
  with_mem_hint(c->policy.mem_hint, [&](auto mh) { launch_step_leg<decltype(mh)::value, SIX>(c, out, imu, q, bc, lin, la); });
}

#if PB_LEG_NS == 15
int pbk_step_leg15(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la)
#else
int pbk_step_leg21(pb_ctx *c, double *out, const double *imu, const double q[4], const StepBcast &bc, const LegIn &lin, const LegStepArgs &la)
#endif
{
  switch (la.mp.mode) {
  case 1: launch_step_leg_mh<1>(c, out, imu, q, bc, lin, la); break;
  case 2: launch_step_leg_mh<2>(c, out, imu, q, bc, lin, la); break;
  default: launch_step_leg_mh<0>(c, out, imu, q, bc, lin, la); break;
  }
  return PB_OK;
}
