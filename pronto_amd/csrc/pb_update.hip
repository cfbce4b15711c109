// pb_update.hip -- launcher of the generic (run-time index list) update of a 15-state batch: k_update_lane_rt<15, M, ORIENT, MH>
// (one lane, the filter in registers) for m <= 4, k_update_coop_rt<M, MH> (two waves per tile, rbis_quad_rt.hpp) for m = 5, 6
// where the one-lane kernel spills; 21 states: pb_update_rt21.hip.  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_update_kernels.hpp"
#include "rbis_quad_rt.hpp"

template <int NS, int M, int MH>
static void launch_update_mh(pb_ctx *c, const IdxArg<M> &ia, const DiagArg<M> &da, const UpdateIn &in)
{
  double *out = update_target(c);
  const double *z = in.z, *R = in.R(), *qm = in.qm;
  const uint8_t *mask = in.mask;
  const int rkind = in.rkind();
  if constexpr (M >= 5) {  // five / six gathered columns beside the covariance do not fit one lane: two waves per tile
    if (two_policy_hint(MH) == MH_STORE_SC1)
      k_update_coop_rt<M, MH_STORE_SC1><<<nblk(c->B), 128, 0, c->stream>>>(c->st, out, c->B, ia, z, R, rkind, da, qm, mask, c->k);
    else
      k_update_coop_rt<M, MH_DEFAULT><<<nblk(c->B), 128, 0, c->stream>>>(c->st, out, c->B, ia, z, R, rkind, da, qm, mask, c->k);
  } else {  // the whole 15-state filter fits one lane's registers: no column gather (k_update_lane_rt)
    if (qm)
      k_update_lane_rt<NS, M, true, MH><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, ia, z, R, rkind, da, qm, mask, c->k);
    else
      k_update_lane_rt<NS, M, false, MH><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, ia, z, R, rkind, da, qm, mask, c->k);
  }
  update_done(c, out);
}

template <int NS, int M>
static void launch_update_m(pb_ctx *c, const int *idx, const UpdateIn &in)
{
  IdxArg<M> ia;
  DiagArg<M> da;
  for (int i = 0; i < M; i++) {
    ia.v[i] = idx[i];
    da.v[i] = in.r_bcast ? in.r_bcast[i] : 0.0;
  }
  with_mem_hint(c->policy.mem_hint, [&](auto mh) { launch_update_mh<NS, M, decltype(mh)::value>(c, ia, da, in); });
}

// family: UPD_LANE_RT (m <= 4) or UPD_COOP_RT (m = 5, 6), as update_choice answers them
int pbk_update15(pb_ctx *c, UpdateFamily family, int m, const int *idx, const UpdateIn &in)
{
  if (family != (m <= 4 ? UPD_LANE_RT : UPD_COOP_RT)) return fail(c, PB_ERR_STATE, "update: no kernel of family %d for m = %d", (int) family, m);
  switch (m) {
    case 1: launch_update_m<15, 1>(c, idx, in); break;
    case 2: launch_update_m<15, 2>(c, idx, in); break;
    case 3: launch_update_m<15, 3>(c, idx, in); break;
    case 4: launch_update_m<15, 4>(c, idx, in); break;
    case 5: launch_update_m<15, 5>(c, idx, in); break;
    case 6: launch_update_m<15, 6>(c, idx, in); break;
    default: return fail(c, PB_ERR_STATE, "update: m must be 1..6");
  }
  LAUNCHCHK(c);
  return PB_OK;
}
