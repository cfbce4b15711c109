// pb_update_ct.hip -- stand-alone indexed (+ orientation) updates whose index list is one the handlers actually produce
// (compile-time core indices, diagonal R): 15 states on the two-role cooperative mapping (k_step_coop with PREDICT = false,
// rbis_coop.hpp), 21 states on the four-wave mapping (k_update_quad, rbis_quad.hpp) -- one coalesced round trip of the
// state, no column gather -- instead of the generic run-time-index kernel k_update.  LegOdoCommon's lin_rot_rate list reaches
// the pass-through angular-velocity states: 15 states take it on the one-lane in-register kernel k_update_lane.  pbk_update, the one
// entry to every update kernel, is here; which kernel it launches is pb_policy.hpp's answer (update_choice).  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_step_kernels.hpp"
#include "rbis_update_kernels.hpp"

template <int NS, int MH, class CORR>
static void launch_ct(pb_ctx *c, double *out, const CorrArgs &ca)
{
  k_step_coop<NS, false, MH, CORR, false><<<nblk(c->B), 128, 0, c->stream>>>(c->st, out, c->B, nullptr, nullptr, nullptr, 0.0, 0.0,
                                                                             0.0, 0.0, c->k, ca);
}
// one of the handlers' lists (CORR) on the mapping the policy named
template <class CORR>
static int launch_list(pb_ctx *c, UpdateFamily family, double *out, const CorrArgs &ca)
{
  if (family == UPD_CT_COOP && c->ns == 15) {
    with_mem_hint(c->policy.mem_hint, [&](auto mh) { launch_ct<15, decltype(mh)::value, CORR>(c, out, ca); });
  } else if (family == UPD_CT_QUAD) {
    with_mem_hint(c->policy.mem_hint, [&](auto mh) {
      k_update_quad<CORR, decltype(mh)::value><<<nblk(c->B), 256, 0, c->stream>>>(c->st, out, c->B, c->k, ca);
    });
  } else {
    if constexpr (CORR::M <= 4) {  // the two-role 21-state mapping (its six-row variants spill: not built, and update_choice never names them)
      with_mem_hint(c->policy.mem_hint, [&](auto mh) { launch_ct<21, decltype(mh)::value, CORR>(c, out, ca); });
    } else {
      return fail(c, PB_ERR_STATE, "update: no six-row kernel on the two-role 21-state mapping");
    }
  }
  return PB_OK;
}

// THE entry to the update kernels: launches the (family, list) update_choice answered (pb_policy.hpp)
int pbk_update(pb_ctx *c, const UpdateChoice &u, int m, const int *idx, const UpdateIn &in)
{
  if (u.family == UPD_WIDE) return pbk_update_wide(c, m, idx, in);
  if (u.family == UPD_LANE_RT || u.family == UPD_COOP_RT) return pbk_update15(c, u.family, m, idx, in);
  if (u.family == UPD_QUAD_RT || u.family == UPD_QUAD_LIST)
    return m <= 3 ? pbk_update21_m123(c, u.family, m, idx, in) : m <= 5 ? pbk_update21_m45(c, u.family, m, idx, in) : pbk_update21_m6(c, u.family, m, idx, in);
  CorrArgs ca;
  ca.z2 = in.z; ca.r2 = in.r_diag; ca.qm2 = in.qm; ca.mask2 = in.mask; ca.rfull = in.r_full;
  if (in.r_bcast)
    for (int i = 0; i < m; i++) ca.rb2[i] = in.r_bcast[i];
  if (u.host_args) {  // one measurement for every filter: host values as kernel arguments
    ca.zbc = 1;
    for (int i = 0; i < m; i++) ca.zb2[i] = in.z_host[i];
    if (in.q_host)
      for (int i = 0; i < 4; i++) ca.qb2[i] = in.q_host[i];
  }
  double *out = update_target(c);
  int rc = PB_OK;
  if (u.family != UPD_LANE_LIST) {
    switch (u.list) {
    case LIST_VEL: rc = launch_list<CorrVel>(c, u.family, out, ca); break;
    case LIST_POS: rc = launch_list<CorrPos>(c, u.family, out, ca); break;
    case LIST_POS_VEL: rc = launch_list<CorrPosVel>(c, u.family, out, ca); break;
    case LIST_POS_ORIENT: rc = launch_list<CorrPosOrient>(c, u.family, out, ca); break;
    case LIST_POS_YAW: rc = launch_list<CorrPosYaw>(c, u.family, out, ca); break;
    case LIST_VEL_YAW: rc = launch_list<CorrVelYaw>(c, u.family, out, ca); break;
    case LIST_YAW: rc = launch_list<CorrYaw>(c, u.family, out, ca); break;
    case LIST_GPF_YAW_POS: rc = launch_list<CorrGpfYawPos>(c, u.family, out, ca); break;
    case LIST_GPF_CHI_POS: rc = launch_list<CorrGpfChiPos>(c, u.family, out, ca); break;
    case LIST_GPF_Z: rc = launch_list<CorrGpfZ>(c, u.family, out, ca); break;
    default: rc = fail(c, PB_ERR_STATE, "update: no compile-time kernel for list %d", u.list); break;
    }
  } else {  // a list that reaches the pass-through states: the one-lane in-register kernel (15 states only)
    with_mem_hint(c->policy.mem_hint, [&](auto mh) {
      k_update_lane<15, 6, IdxVelOmega, decltype(mh)::value><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, c->k, ca);
    });
  }
  if (rc) return rc;
  LAUNCHCHK(c);
  update_done(c, out);
  return PB_OK;
}
