// mav_state_est_gpf.hpp -- opt-in: the laser GPF measurement (state-estimator/src/gpf/gpf.hpp:53-192, rbis_gpf_update.cpp:28-76,
// laser_gpf_lib.cpp) behind the reference's class names, on the pb_gpf_* family (include/pronto_batch.h).
//
// Why a header of its own: the classes below call pb_gpf_* and pb_update_indexed_wide, and a program that includes mav_state_est.hpp /
// mav_state_est_batch.hpp alone must keep linking against exactly the pb_* functions those two use (tests/cpp/abi_recorder.cpp stands in
// for the library there).  Include this header instead of mav_state_est_wide.hpp and register LaserGPFHandler for the scan channel.
//
// Out of scope here, as in the C ABI: octomap loading and blurring (the map is a dense voxel grid), the planar-lidar projection,
// beam_skip / spatial decimation and the frames tree -- the handler's message is a block of already projected scan points in the body
// frame --, lcmgl drawing and publishing GPF_MEASUREMENT.
#pragma once

#include "mav_state_est_wide.hpp"

namespace MavStateEst {

// GPFLikelihoodInterface<T>::likelihoodFunction (gpf.hpp:21-38) for all K samples of all filters at once: pose_dev [K][7][B] (position
// xyz, quaternion wxyz: RBIS::getBotTrans of every sample state) -> loglik_dev [K][B], both device memory.  Returns a pb_status.
class GPFLikelihoodInterface {
public:
  virtual ~GPFLikelihoodInterface() {}
  virtual int logLikelihoods(pb_ctx *ctx, int K, const double *pose_dev, double *loglik_dev) = 0;
};

// the map of the built-in likelihood: what pb_gpf_grid_set takes, handed to the context by the first likelihood that needs it
struct GridMap {
  double origin[3] = { 0, 0, 0 }, resolution = 1.0, unknown_loglike = 0.0, cov_scaling = 1.0;
  int dims[3] = { 1, 1, 1 };     // nx, ny, nz
  std::vector<double> values;    // [nz][ny][nx]: what -node->getLogOdds() would return
  std::shared_ptr<bool> on_alive;  // the lifetime token of the estimator whose context holds it (a context's ADDRESS can come back
                                   // with the next estimator, which has no map yet)
};

// LaserLikelihoodInterface::evaluateScanLogLikelihood (LaserLikelihoodInterface.cpp:5-77) of ONE scan over the grid: the two grid calls.
// The scan's points are owned (host: [3 n] for PB_HOST_BROADCAST, [3 n][B] for PB_HOST) or read in place (PB_DEVICE).
class GridLikelihood : public GPFLikelihoodInterface {
public:
  std::shared_ptr<GridMap> map;
  std::vector<double> owned_points;
  const double *points;
  int n_points, points_mem;
  std::shared_ptr<bool> ctx_alive;  // MavStateEstimator::ctx_alive of the estimator this scan was made for
  GridLikelihood(std::shared_ptr<GridMap> map_, const BatchArray &pts, int n_points_, int B, std::shared_ptr<bool> ctx_alive_)
      : map(std::move(map_)), points(pts.p), n_points(n_points_), points_mem(pts.mem), ctx_alive(std::move(ctx_alive_))
  {
    if (pts.mem != PB_DEVICE) {
      owned_points = own_rows(pts, (size_t) 3 * n_points, B);
      points = owned_points.data();
    }
  }
  int logLikelihoods(pb_ctx *ctx, int K, const double *pose_dev, double *loglik_dev) override
  {
    if (map->on_alive != ctx_alive) {
      const int rc = pb_gpf_grid_set(ctx, map->origin, map->resolution, map->dims, map->values.data(), map->unknown_loglike, map->cov_scaling);
      if (rc != PB_OK) return rc;
      map->on_alive = ctx_alive;
    }
    return pb_gpf_grid_loglik(ctx, K, pose_dev, n_points, points, points_mem, loglik_dev);
  }
};

// RBISLaserGPFMeasurement (rbis_gpf_update.cpp:28-76): sample -> likelihood -> effective measurement -> indexed update, all on the
// device.  The normals come from pb_gpf_normals(seed, stream_id = this update's own serial number), so an update the history re-applies
// after a late arrival draws the same xi and is deterministic.  The reference redraws on every application (gpf.hpp:92): there a replayed
// history ends at another posterior than the one it first computed.
class RBISGPFMeasurement : public RBISUpdateInterface {
public:
  std::vector<int> index;
  int K, B;
  double max_weight_proportion;
  uint64_t seed;
  uint32_t stream_id;
  std::shared_ptr<GPFLikelihoodInterface> likelihood;
  std::shared_ptr<DevicePool> pool;  // blocks of scratch_bytes(m, K, B)
  static size_t scratch_bytes(int m, int K, int B)
  {
    return sizeof(double) * (size_t) B * ((size_t) K * (2 * m + 8) + m + m * m) + sizeof(int32_t) * (size_t) B;
  }
  RBISGPFMeasurement(const std::vector<int> &index_, int K_, int B_, double max_weight_proportion_, uint64_t seed_, uint32_t stream_id_,
                     std::shared_ptr<GPFLikelihoodInterface> likelihood_, std::shared_ptr<DevicePool> pool_, sensor_enum sensor_id_, int64_t utime_)
      : RBISUpdateInterface(sensor_id_, utime_), index(index_), K(K_), B(B_), max_weight_proportion(max_weight_proportion_), seed(seed_),
        stream_id(stream_id_), likelihood(std::move(likelihood_)), pool(std::move(pool_)) {}
  int updateFilter(pb_ctx *ctx) override
  {
    const int m = (int) index.size();
    // (the block goes back to the pool when this call returns: stream order keeps the next user behind the kernels enqueued here)
    const std::shared_ptr<DeviceBlock> blk = take_block(pool);
    if (!blk) return PB_ERR_HIP;
    const size_t Bz = (size_t) B, Kz = (size_t) K;
    double *xi = (double *) blk->p, *delta = xi + Kz * m * Bz, *pose = delta + Kz * m * Bz, *ll = pose + Kz * 7 * Bz, *z = ll + Kz * Bz,
           *R = z + (size_t) m * Bz;
    int32_t *status = (int32_t *) (R + (size_t) m * m * Bz);
    int rc = pb_gpf_normals(ctx, seed, stream_id, K * m, xi);
    if (rc == PB_OK) rc = pb_gpf_sample(ctx, m, index.data(), K, xi, delta, pose);
    if (rc == PB_OK) rc = likelihood->logLikelihoods(ctx, K, pose, ll);
    if (rc == PB_OK) rc = pb_gpf_measurement(ctx, m, index.data(), K, delta, ll, max_weight_proportion, z, R, status);
    if (rc == PB_OK) rc = pb_update_indexed_wide(ctx, m, index.data(), z, R, PB_R_FULL, nullptr, nullptr, PB_DEVICE);
    return rc;
  }
};

// one scan, already projected: n_points points in the body frame, rows x0, y0, z0, x1, ... -- [3 n] (PB_HOST_BROADCAST: one robot's
// scan for every filter) or [3 n][B] (PB_HOST, PB_DEVICE).  A point whose x is not finite is skipped.
namespace msgs {
struct scan_points_t {
  int64_t utime = 0;
  int n_points = 0;
  BatchArray points;
};
}  // namespace msgs

// LaserGPFHandler (laser_gpf_lib.cpp, the handler of sensor_handlers.cpp): state_estimator.laser_gpf.{gpf_num_samples, gpf_substate,
// max_weight_proportion, unknown_loglike, sigma_scaling} as the reference reads them (cov_scaling = sigma_scaling^2); the substate
// lists are laser_gpf_lib.cpp:91-116.  The map's unknown_loglike / cov_scaling are set from the keys.  Optional key of this build:
// state_estimator.laser_gpf.seed (default 0), the Philox key of every update's normals.
class LaserGPFHandler {
public:
  std::vector<int> indices;
  int num_samples;
  double max_weight_proportion;
  uint64_t seed;
  uint32_t next_serial = 0;
  std::shared_ptr<GridMap> map;
  LaserGPFHandler(BotParam *param, std::shared_ptr<GridMap> map_) : map(std::move(map_))
  {
    num_samples = (int) bot_param_get_int_or_fail(param, "state_estimator.laser_gpf.gpf_num_samples");
    const std::string substate = bot_param_get_str_or_fail(param, "state_estimator.laser_gpf.gpf_substate");
    max_weight_proportion = bot_param_get_double_or_fail(param, "state_estimator.laser_gpf.max_weight_proportion");
    map->unknown_loglike = bot_param_get_double_or_fail(param, "state_estimator.laser_gpf.unknown_loglike");
    map->cov_scaling = bot_sq(bot_param_get_double_or_fail(param, "state_estimator.laser_gpf.sigma_scaling"));
    seed = (uint64_t) bot_param_get_int_or(param, "state_estimator.laser_gpf.seed", 0);
    if (substate == "pos_only") indices = { 9, 10, 11 };
    else if (substate == "pos_yaw") indices = { 8, 9, 10, 11 };
    else if (substate == "pos_chi") indices = { 6, 7, 8, 9, 10, 11 };
    else if (substate == "all_states") indices = { 3, 4, 5, 6, 7, 8, 9, 10, 11 };
    else if (substate == "z_only") indices = { 11 };
    else {
      fprintf(stderr, "ERROR: LaserGPFHandler: unknown gpf_substate '%s'\n", substate.c_str());
      exit(1);  // the reference's fatal error
    }
    fprintf(stderr, "LaserGpf is using the %s substate mode\n", substate.c_str());
  }
  RBISUpdateInterface *processMessage(const msgs::scan_points_t *msg, MavStateEstimator *est)
  {
    if (num_samples < 1) {
      fprintf(stderr, "LaserGPFHandler: gpf_num_samples = %d, no measurement\n", num_samples);
      return nullptr;
    }
    const int m = (int) indices.size();
    if (!pool_ || pool_->alive != est->ctx_alive)
      pool_ = std::make_shared<DevicePool>(est->ctx, est->ctx_alive, RBISGPFMeasurement::scratch_bytes(m, num_samples, est->B));
    return new RBISGPFMeasurement(indices, num_samples, est->B, max_weight_proportion, seed, next_serial++,
                                  std::make_shared<GridLikelihood>(map, msg->points, msg->n_points, est->B, est->ctx_alive), pool_, RBISUpdateInterface::laser_gpf,
                                  msg->utime);
  }
private:
  std::shared_ptr<DevicePool> pool_;
};

}  // namespace MavStateEst
