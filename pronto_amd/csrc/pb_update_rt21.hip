// pb_update_rt21.hip -- launcher of the generic (run-time index list) update of a 21-state batch: k_update_quad_rt<M, MH>
// (rbis_quad_rt.hpp).  The kernel is expensive to compile (a 21-way column pick per measurement and wave), so the six m are
// spread over three objects built in parallel: -DPB_UPD_MSET=0 (m = 1, 2, 3), 1 (m = 4, 5), 2 (m = 6); see pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_quad_rt.hpp"

template <int M>
static int launch_rt21(pb_ctx *c, UpdateFamily family, const int *idx, const UpdateIn &in)
{
  if (family != UPD_QUAD_RT) return fail(c, PB_ERR_STATE, "update: no 21-state kernel of family %d for m = %d", (int) family, M);
  IdxArg<M> ia;
  DiagArg<M> da;
  for (int i = 0; i < M; i++) {
    if (idx[i] < 0 || idx[i] > 20) return fail(c, PB_ERR_ARG, "update: index %d out of range", idx[i]);
    ia.v[i] = idx[i];
    da.v[i] = in.r_bcast ? in.r_bcast[i] : 0.0;
  }
  double *out = update_target(c);
  if (two_policy_hint(c->policy.mem_hint) == MH_STORE_SC1)
    k_update_quad_rt<M, MH_STORE_SC1><<<nblk(c->B), 256, 0, c->stream>>>(c->st, out, c->B, ia, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
  else
    k_update_quad_rt<M, MH_DEFAULT><<<nblk(c->B), 256, 0, c->stream>>>(c->st, out, c->B, ia, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
  LAUNCHCHK(c);
  update_done(c, out);
  return PB_OK;
}

#if PB_UPD_MSET == 0
int pbk_update21_m123(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in)
{
  if (m == 1) return launch_rt21<1>(c, family, idx, in);
  if (m == 2) return launch_rt21<2>(c, family, idx, in);
  return launch_rt21<3>(c, family, idx, in);
}
#elif PB_UPD_MSET == 1
int pbk_update21_m45(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in)
{
  if (m == 4) return launch_rt21<4>(c, family, idx, in);
  return launch_rt21<5>(c, family, idx, in);
}
#else
int pbk_update21_m6(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in)
{
  if (family == UPD_QUAD_LIST) {  // LegOdoCommon's lin_rot_rate list [3,4,5,0,1,2] (update_choice)
    DiagArg<6> da;
    for (int i = 0; i < 6; i++) da.v[i] = in.r_bcast ? in.r_bcast[i] : 0.0;
    double *out = update_target(c);
    if (two_policy_hint(c->policy.mem_hint) == MH_STORE_SC1)
      k_update_quad_list<MH_STORE_SC1, 3, 4, 5, 0, 1, 2><<<nblk(c->B), 256, 0, c->stream>>>(c->st, out, c->B, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
    else
      k_update_quad_list<MH_DEFAULT, 3, 4, 5, 0, 1, 2><<<nblk(c->B), 256, 0, c->stream>>>(c->st, out, c->B, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
    LAUNCHCHK(c);
    update_done(c, out);
    return PB_OK;
  }
  return launch_rt21<6>(c, family, idx, in);
}
#endif
