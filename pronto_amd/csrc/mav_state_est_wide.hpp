// mav_state_est_wide.hpp -- opt-in: indexed measurements of seven to nine rows (the GPF's all_states list, velocity + chi + position,
// rgbd_gpf_lib.cpp:86-91) behind the reference's class names.  The reference's RBISIndexedMeasurement takes an index list of any length
// (rbis.cpp:160-217) and IndexedMeasurementHandler passes on whatever pronto::indexed_measurement_t carries (sensor_handlers.cpp:576-582);
// pb_update_indexed / pb_update_indexed_orient stop at six rows, pb_update_indexed_wide at nine (include/pronto_batch.h).
//
// Why a header of its own: the classes below call pb_update_indexed_wide, and a program that includes mav_state_est.hpp /
// mav_state_est_batch.hpp alone must keep linking against exactly the pb_* functions those two use (tests/cpp/abi_recorder.cpp stands in
// for the library there).  Include this header instead of mav_state_est_batch.hpp and register WideIndexedMeasurementHandler where
// IndexedMeasurementHandler was registered; nothing else changes.
#pragma once

#include "mav_state_est_batch.hpp"

namespace MavStateEst {

// RBISIndexedMeasurement for up to PB_UPDATE_WIDE_MAX_ROWS rows.  Payloads, device blocks and the mask are the base class's; through
// MavStateEstimator::addUpdate it enters the history, is checkpointed and re-applied like any measurement.
class RBISWideIndexedMeasurement : public RBISIndexedMeasurement {
public:
  using RBISIndexedMeasurement::RBISIndexedMeasurement;
  int updateFilter(pb_ctx *ctx) override
  {
    const int rc = resolve(ctx, nullptr);
    if (rc != PB_OK) return rc;
    return pb_update_indexed_wide(ctx, (int) index.size(), index.data(), measurement.p, measurement_cov, r_kind, nullptr, mask, measurement.mem);
  }
};

class RBISWideIndexedPlusOrientationMeasurement : public RBISIndexedPlusOrientationMeasurement {
public:
  using RBISIndexedPlusOrientationMeasurement::RBISIndexedPlusOrientationMeasurement;
  int updateFilter(pb_ctx *ctx) override
  {
    return pb_update_indexed_wide(ctx, (int) index.size(), index.data(), measurement.p, measurement_cov, r_kind, orientation.p, mask,
                                  measurement.mem);
  }
};

// IndexedMeasurementHandler for messages of up to nine rows.  Up to six rows: exactly what IndexedMeasurementHandler returns (same
// class, same fields); seven to nine: the wide update, for host and PB_DEVICE messages alike; more: NULL, reported.
class WideIndexedMeasurementHandler {
public:
  explicit WideIndexedMeasurementHandler(RBISUpdateInterface::sensor_enum this_sensor) : narrow(this_sensor), indexed_sensor(this_sensor) {}
  RBISUpdateInterface *processMessage(const msgs::indexed_measurement_t *msg, MavStateEstimator *est)
  {
    const int m = (int) msg->z_indices.size();
    if (m <= 6) return narrow.processMessage(msg, est);
    if (m > PB_UPDATE_WIDE_MAX_ROWS) {
      fprintf(stderr, "WideIndexedMeasurementHandler: %d rows (at most %d)\n", m, PB_UPDATE_WIDE_MAX_ROWS);
      return nullptr;
    }
    // sensor_handlers.cpp:576-582, as IndexedMeasurementHandler: the update owns a copy of host data, device blocks stay where they are
    if (msg->z_effective.mem == PB_DEVICE)
      return new RBISWideIndexedMeasurement(msg->z_indices, msg->z_effective, msg->R_effective, PB_R_FULL, nullptr, indexed_sensor, msg->utime);
    const int mem = msg->z_effective.mem, B = est ? est->B : 1;
    auto *u = new RBISWideIndexedMeasurement(msg->z_indices, own_rows(msg->z_effective, (size_t) m, B),
                                             own_rows(BatchArray(msg->R_effective, mem), (size_t) m * m, B), PB_R_FULL, std::vector<uint8_t>(),
                                             indexed_sensor, msg->utime);
    u->measurement.mem = u->cov_mem = mem;
    return u;
  }
  bool processMessageInit(const msgs::indexed_measurement_t *msg, const std::map<std::string, bool> &sensors_initialized, const RBIS &default_state,
                          const RBIM &default_cov, RBIS &init_state, RBIM &init_cov)
  {
    return narrow.processMessageInit(msg, sensors_initialized, default_state, default_cov, init_state, init_cov);
  }
private:
  IndexedMeasurementHandler narrow;
  RBISUpdateInterface::sensor_enum indexed_sensor;
};

}  // namespace MavStateEst
