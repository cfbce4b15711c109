// mav_state_est_flow.hpp -- opt-in: the optical-flow handler (OpticalFlowHandler, sensor_handlers.cpp:726-763) and its four-row
// unscented update (RBISOpticalFlowMeasurement, rbis_update_interface.hpp:128-154, .cpp:109-260) behind the reference's class names,
// on pb_flow_set_camera / pb_update_optical_flow (include/pronto_batch.h).
//
// Why a header of its own: the classes below call the two pb_flow functions, and a program that includes mav_state_est.hpp /
// mav_state_est_batch.hpp alone must keep linking against exactly the pb_* functions those two use (tests/cpp/abi_recorder.cpp stands in
// for the library there).  Include this header instead of mav_state_est_batch.hpp and register OpticalFlowHandler for the flow channel.
//
// An update owns its message (host values) or names a device block that stays what it was, and the kernel draws nothing at random: an
// update that the history re-applies after a late arrival is deterministic by construction.
// Out of scope: publishing OPTICAL_FLOW_PSEUDO (:140-158) -- pb_update_optical_flow's zhat_out is that message's content.
#pragma once

#include "mav_state_est_batch.hpp"

namespace MavStateEst {

namespace msgs {
// pronto::optical_flow_t (pronto_optical_flow_t.lcm) for the batch.  flow: rows ux, uy, theta, scale, alpha1, alpha2, gamma -- the
// order of the measurement vector (sensor_handlers.cpp:748-755), not of the wire type, where scale comes before theta -- as [7]
// (PB_HOST_BROADCAST: one robot's message for every filter) or [7][B] (PB_HOST, PB_DEVICE).  dt, conf_rs and conf_xy are not read
// by the handler.  mask [B] (host with PB_HOST, device with PB_DEVICE) or NULL: 0 = no message for this filter.
struct optical_flow_t {
  int64_t utime = 0;
  BatchArray flow;
  const uint8_t *mask = nullptr;
  double one[7] = { 0, 0, 0, 0, 0, 0, 0 };  // storage of a single robot's message (set)
  void set(double ux, double uy, double theta, double scale, double alpha1, double alpha2, double gamma)
  {
    const double v[7] = { ux, uy, theta, scale, alpha1, alpha2, gamma };
    for (int i = 0; i < 7; i++) one[i] = v[i];
    flow = BatchArray(one, PB_HOST_BROADCAST);
  }
};
}  // namespace msgs

// RBISOpticalFlowMeasurement.  The reference's constructor arguments (rbis_update_interface.hpp:143-150): z_meas [4], cov_xyrs 4 x 4
// column-major, body_to_cam_trans [3], body_to_cam_rot 3 x 3 column-major as the Eigen matrix holds it -- its columns are zeta1, zeta2,
// eta --, alpha1, alpha2, gamma.  That is one robot's message for every filter; the second constructor takes a message block.
// flags: pb_update_optical_flow's (default 0, the reference).
class RBISOpticalFlowMeasurement : public RBISUpdateInterface {
public:
  std::vector<double> owned_flow;  // host messages: [7] or [7][B]
  BatchArray flow;
  std::vector<uint8_t> owned_mask;
  const uint8_t *mask = nullptr;
  double cov_xyrs[16];
  double r[3], zeta1[3], zeta2[3], eta[3];
  int B = 1, flags = 0;
  RBISOpticalFlowMeasurement(const double z_meas[4], const double cov_xyrs_[16], const double body_to_cam_trans[3], const double body_to_cam_rot[9],
                             double alpha1, double alpha2, double gamma, sensor_enum sensor_id_, int64_t utime_)
      : RBISUpdateInterface(sensor_id_, utime_)
  {
    owned_flow = { z_meas[0], z_meas[1], z_meas[2], z_meas[3], alpha1, alpha2, gamma };
    flow = BatchArray(owned_flow.data(), PB_HOST_BROADCAST);
    set_camera(cov_xyrs_, body_to_cam_trans, body_to_cam_rot);
  }
  RBISOpticalFlowMeasurement(const BatchArray &flow_block, const uint8_t *mask_, int B_, const double cov_xyrs_[16], const double body_to_cam_trans[3],
                             const double body_to_cam_rot[9], sensor_enum sensor_id_, int64_t utime_)
      : RBISUpdateInterface(sensor_id_, utime_), flow(flow_block), mask(mask_), B(B_)
  {
    if (flow.mem != PB_DEVICE) {
      owned_flow = own_rows(flow, 7, B);
      flow = BatchArray(owned_flow.data(), flow.mem);
      owned_mask = own_mask(mask, flow.mem, B);
      mask = owned_mask.empty() ? nullptr : owned_mask.data();
    }
    set_camera(cov_xyrs_, body_to_cam_trans, body_to_cam_rot);
  }
  int updateFilter(pb_ctx *ctx) override
  {
    int rc = pb_flow_set_camera(ctx, r, zeta1, zeta2, eta);
    if (rc != PB_OK) return rc;
    bool diagonal = true;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) diagonal = diagonal && (i == j || cov_xyrs[j * 4 + i] == 0.0);
    if (diagonal) {  // the handler's (sensor_handlers.cpp:742): four host values serve every memory space
      const double d[4] = { cov_xyrs[0], cov_xyrs[5], cov_xyrs[10], cov_xyrs[15] };
      return pb_update_optical_flow(ctx, flow.p, d, PB_R_DIAG_BROADCAST, mask, flow.mem, flags, nullptr, nullptr);
    }
    if (flow.mem == PB_HOST_BROADCAST) return pb_update_optical_flow(ctx, flow.p, cov_xyrs, PB_R_FULL, mask, flow.mem, flags, nullptr, nullptr);
    if (flow.mem != PB_HOST) return PB_ERR_ARG;  // a full host covariance beside a device message: the caller passes blocks to the C ABI itself
    std::vector<double> full((size_t) 16 * B);
    for (int i = 0; i < 16; i++)
      for (int b = 0; b < B; b++) full[(size_t) i * B + b] = cov_xyrs[i];
    return pb_update_optical_flow(ctx, flow.p, full.data(), PB_R_FULL, mask, PB_HOST, flags, nullptr, nullptr);
  }

private:
  void set_camera(const double cov_xyrs_[16], const double trans[3], const double rot[9])
  {
    for (int i = 0; i < 16; i++) cov_xyrs[i] = cov_xyrs_[i];
    for (int i = 0; i < 3; i++) {
      r[i] = trans[i];
      zeta1[i] = rot[i];  // col(0), rbis_update_interface.hpp:146-148
      zeta2[i] = rot[3 + i];
      eta[i] = rot[6 + i];
    }
  }
};

// libbot's bot_quat_to_matrix, row-major: what bot_trans_get_rot_mat_3x3 writes (sensor_handlers.cpp:730)
inline void bot_trans_get_rot_mat_3x3(const BotTrans *t, double rot[9])
{
  const double *q = t->rot_quat;
  const double norm = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (fabs(norm) < 1e-10) {
    for (int i = 0; i < 9; i++) rot[i] = 0.0;
    return;
  }
  const double in = 1 / norm;
  const double w = q[0] * in, x = q[1] * in, y = q[2] * in, z = q[3] * in;
  const double w2 = q[0] * w, x2 = q[1] * x, y2 = q[2] * y, z2 = q[3] * z;
  const double xy = 2 * q[1] * y, xz = 2 * q[1] * z, yz = 2 * q[2] * z, wx = 2 * q[0] * x, wy = 2 * q[0] * y, wz = 2 * q[0] * z;
  rot[0] = w2 + x2 - y2 - z2; rot[1] = xy - wz;           rot[2] = xz + wy;
  rot[3] = xy + wz;           rot[4] = w2 - x2 + y2 - z2; rot[5] = yz - wx;
  rot[6] = xz - wy;           rot[7] = yz + wx;           rot[8] = w2 - x2 - y2 + z2;
}

// OpticalFlowHandler: state_estimator.optical_flow.{r_ux, r_uy, r_r, r_s}, squared, as the diagonal of cov_xyrs (:735-742).  The
// body -> camera transform comes from the caller, as InsHandler takes ins_to_body (the reference asks BotFrames for "body" to "camera",
// :728).  bot_trans_get_rot_mat_3x3 fills the data of a column-major Eigen matrix row-major (:730), so the nine doubles read as that
// Eigen matrix are libbot's rotation transposed, and its columns -- zeta1, zeta2, eta -- are the ROWS of the body -> camera rotation.
class OpticalFlowHandler {
public:
  BotTrans body_to_cam;
  double body_to_cam_trans[3], body_to_cam_rot[9];
  double cov_xyrs[16];
  int flags = 0;  // pb_update_optical_flow's, for every update this handler makes
  OpticalFlowHandler(BotParam *param, const BotTrans *body_to_cam_) : body_to_cam(*body_to_cam_)
  {
    for (int i = 0; i < 3; i++) body_to_cam_trans[i] = body_to_cam.trans_vec[i];
    bot_trans_get_rot_mat_3x3(&body_to_cam, body_to_cam_rot);
    const double rr[4] = { bot_param_get_double_or_fail(param, "state_estimator.optical_flow.r_ux"),
                           bot_param_get_double_or_fail(param, "state_estimator.optical_flow.r_uy"),
                           bot_param_get_double_or_fail(param, "state_estimator.optical_flow.r_r"),
                           bot_param_get_double_or_fail(param, "state_estimator.optical_flow.r_s") };
    for (int i = 0; i < 16; i++) cov_xyrs[i] = 0.0;
    for (int i = 0; i < 4; i++) cov_xyrs[i * 5] = bot_sq(rr[i]);
  }
  RBISUpdateInterface *processMessage(const msgs::optical_flow_t *msg, MavStateEstimator *est)
  {
    auto *u = new RBISOpticalFlowMeasurement(msg->flow, msg->mask, est ? est->B : 1, cov_xyrs, body_to_cam_trans, body_to_cam_rot,
                                             RBISUpdateInterface::optical_flow, msg->utime);
    u->flags = flags;
    return u;
  }
};

}  // namespace MavStateEst
