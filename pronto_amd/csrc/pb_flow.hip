// pb_flow.hip -- the optical-flow sigma-point update of the C ABI (pb_flow_set_camera, pb_update_optical_flow) and the launcher of
// k_update_flow<NS, MH> (rbis_flow_kernels.hpp).  The layout is fixed -- always rows 0 ... 11 -- so there is no policy: one kernel,
// instantiated for the state size and, like pb_update_wide.hip, for two cache policies (non-temporal streaming falls back to the
// default one).  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_flow_kernels.hpp"

static_assert(PB_FLOW_HEAD_QUAT == FLOW_HEAD_QUAT, "the flag of the header is the flag of the lane function");

extern "C" int pb_flow_set_camera(pb_ctx *c, const double body_to_cam_trans[3], const double zeta1[3], const double zeta2[3],
                                  const double eta[3])
{
  CALL(c, 0);
  if (!body_to_cam_trans || !zeta1 || !zeta2 || !eta) return fail(c, PB_ERR_ARG, "pb_flow_set_camera: NULL argument");
  for (int i = 0; i < 3; i++) {
    c->flow_cam.r[i] = body_to_cam_trans[i];
    c->flow_cam.zeta1[i] = zeta1[i];
    c->flow_cam.zeta2[i] = zeta2[i];
    c->flow_cam.eta[i] = eta[i];
  }
  c->flow_wt = flow_weights();  // rbis_update_interface.cpp:199-206, on the host, once
  c->flow_cam_on = true;
  return PB_OK;
}

extern "C" int pb_update_optical_flow(pb_ctx *c, const double *flow_block, const double *R, int r_kind, const uint8_t *mask, int mem,
                                      int flags, double *zhat_out, int32_t *status_out)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  if (!c->flow_cam_on) return fail(c, PB_ERR_STATE, "pb_update_optical_flow before pb_flow_set_camera");
  if (!flow_block || !R) return fail(c, PB_ERR_ARG, "pb_update_optical_flow: NULL input");
  if (flags & ~PB_FLOW_HEAD_QUAT) return fail(c, PB_ERR_ARG, "pb_update_optical_flow: unknown flags %d", flags);
  const size_t B = (size_t) c->B;
  // (every input block goes through one 32-bit-ranged buffer descriptor)
  if ((unsigned long long) B * 16ull * 8ull >= (1ull << 32)) return fail(c, PB_ERR_ARG, "pb_update_optical_flow: batch %d too large", c->B);
  size_t rbytes;
  if (mem == PB_HOST_BROADCAST && r_kind == PB_R_DIAG) r_kind = PB_R_DIAG_BROADCAST;  // the same thing, without a fill
  if (r_kind == PB_R_DIAG_BROADCAST) rbytes = 0;
  else if (r_kind == PB_R_DIAG) rbytes = sizeof(double) * FLOW_M * B;
  else if (r_kind == PB_R_FULL) rbytes = sizeof(double) * FLOW_M * FLOW_M * B;
  else return fail(c, PB_ERR_ARG, "pb_update_optical_flow: bad r_kind %d", r_kind);
  DiagArg<FLOW_M> rb;
  for (int i = 0; i < FLOW_M; i++) rb.v[i] = r_kind == PB_R_DIAG_BROADCAST ? R[i] : 0.0;
  Part p[3] = { { flow_block, sizeof(double) * 7 * B, 0 }, { r_kind == PB_R_DIAG_BROADCAST ? nullptr : R, rbytes, 0 }, { mask, B, 0 } };
  if (int rc = stage_in(c, mem, p, 3)) return rc;
  const double *flow = (const double *) p[0].dev, *Rd = (const double *) p[1].dev;
  const uint8_t *md = (const uint8_t *) p[2].dev;
  double *out = update_target(c);
  with_ns(c->ns, [&](auto NS) {
    constexpr int ns = decltype(NS)::value;
    if (two_policy_hint(c->policy.mem_hint) == MH_STORE_SC1)
      k_update_flow<ns, MH_STORE_SC1><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, flow, Rd, r_kind, rb, md, c->flow_cam, c->flow_wt, flags,
                                                                       zhat_out, status_out, c->k);
    else
      k_update_flow<ns, MH_DEFAULT><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, flow, Rd, r_kind, rb, md, c->flow_cam, c->flow_wt, flags,
                                                                     zhat_out, status_out, c->k);
  });
  LAUNCHCHK(c);
  update_done(c, out);
  return PB_OK;
}
