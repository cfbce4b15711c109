// pb_gpf.hip -- the GPF measurement family of the C ABI (pb_gpf_*) and the launchers of its kernels (rbis_gpf_kernels.hpp): normals,
// samples of each filter's marginal with their poses, the fit of the particle clouds with the effective measurement, and the built-in
// voxel-grid likelihood.  The layouts are fixed, so there is no policy: one kernel per entry point, instantiated for the state size and
// the number of rows.  None of the calls writes the filter: applying z_eff / R_eff is pb_update_indexed_wide's.  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_gpf_kernels.hpp"

static_assert(GPF_MAX_ROWS == PB_UPDATE_WIDE_MAX_ROWS, "the fit's outputs are pb_update_indexed_wide's inputs");

// f(NS, M) with both as compile-time constants
template <class F>
static void with_ns_m(int ns, int m, F f)
{
  with_ns(ns, [&](auto NS) {
    static_for<GPF_MAX_ROWS>([&](auto I) {
      if (m == decltype(I)::value + 1) f(NS, std::integral_constant<int, decltype(I)::value + 1>());
    });
  });
}

static int gpf_check(pb_ctx *c, const char *who, int m, const int *idx, int K)
{
  if (m < 1 || m > GPF_MAX_ROWS) return fail(c, PB_ERR_ARG, "%s: m must be 1..%d (got %d)", who, GPF_MAX_ROWS, m);
  if (!idx) return fail(c, PB_ERR_ARG, "%s: NULL index list", who);
  if (int rc = pbk_check_indices(c, m, idx)) return rc;
  if (K < 1) return fail(c, PB_ERR_ARG, "%s: K must be at least 1 (got %d)", who, K);
  if ((unsigned long long) K * 81ull * (unsigned long long) c->B >= (1ull << 40)) return fail(c, PB_ERR_ARG, "%s: %d samples of %d filters are too many", who, K, c->B);
  return PB_OK;
}

extern "C" int pb_gpf_normals(pb_ctx *c, uint64_t seed, uint32_t stream_id, int rows, double *out_dev)
{
  CALL(c, 0);
  if (rows < 1 || !out_dev) return fail(c, PB_ERR_ARG, "pb_gpf_normals: rows must be at least 1 and the output block not NULL");
  const int pairs = (rows + 1) / 2;
  k_gpf_normals<<<dim3(nblk(c->B), std::min(pairs, 65535)), 64, 0, c->stream>>>(seed, stream_id, rows, c->B, out_dev);
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_gpf_sample(pb_ctx *c, int m, const int *idx, int K, const double *xi_dev, double *delta_out_dev, double *pose_out_dev)
{
  CALL(c, NEEDS_STATE);
  if (int rc = gpf_check(c, "pb_gpf_sample", m, idx, K)) return rc;
  if (!xi_dev || !delta_out_dev || !pose_out_dev) return fail(c, PB_ERR_ARG, "pb_gpf_sample: NULL block");
  const int chunks = (K + GPF_SAMPLE_CHUNK - 1) / GPF_SAMPLE_CHUNK;
  if (chunks > 65535) return fail(c, PB_ERR_ARG, "pb_gpf_sample: at most %d samples", 65535 * GPF_SAMPLE_CHUNK);
  with_ns_m(c->ns, m, [&](auto NS, auto M) {
    k_gpf_sample<decltype(NS)::value, decltype(M)::value><<<dim3(nblk(c->B), chunks), 64, 0, c->stream>>>(
        c->st, c->B, make_gpf_tab<decltype(NS)::value, decltype(M)::value>(idx), K, xi_dev, delta_out_dev, pose_out_dev, c->k.chi_tol);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_gpf_measurement(pb_ctx *c, int m, const int *idx, int K, const double *delta_dev, const double *loglik_dev,
                                  double max_weight_proportion, double *z_eff_out_dev, double *R_eff_out_dev, int32_t *status_out_dev)
{
  CALL(c, NEEDS_STATE);
  if (int rc = gpf_check(c, "pb_gpf_measurement", m, idx, K)) return rc;
  if (!delta_dev || !loglik_dev || !z_eff_out_dev || !R_eff_out_dev || !status_out_dev) return fail(c, PB_ERR_ARG, "pb_gpf_measurement: NULL block");
  with_ns_m(c->ns, m, [&](auto NS, auto M) {
    k_gpf_fit<decltype(NS)::value, decltype(M)::value><<<nblk(c->B), 256, 0, c->stream>>>(
        c->st, c->B, make_gpf_tab<decltype(NS)::value, decltype(M)::value>(idx), K, delta_dev, loglik_dev, max_weight_proportion, z_eff_out_dev,
        R_eff_out_dev, status_out_dev);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_gpf_grid_set(pb_ctx *c, const double origin[3], double resolution, const int dims[3], const double *values_host,
                               double unknown_loglike, double cov_scaling)
{
  CALL(c, 0);
  if (!origin || !dims || !values_host) return fail(c, PB_ERR_ARG, "pb_gpf_grid_set: NULL argument");
  if (!(resolution > 0.0) || !(cov_scaling > 0.0)) return fail(c, PB_ERR_ARG, "pb_gpf_grid_set: resolution and cov_scaling must be positive");
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || (unsigned long long) dims[0] * dims[1] * dims[2] >= (1ull << 31))
    return fail(c, PB_ERR_ARG, "pb_gpf_grid_set: bad dimensions %d x %d x %d", dims[0], dims[1], dims[2]);
  const size_t n = (size_t) dims[0] * dims[1] * dims[2];
  if (n > c->gpf_grid_n) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->gpf_grid_n = 0;
    c->gpf_grid_on = false;
    HIPCHK(c, dev_release(c, c->gpf_grid));
    if (int rc = dev_alloc(c, c->gpf_grid, n)) return rc;
    c->gpf_grid_n = n;
  }
  HIPCHK(c, hipMemcpyAsync(c->gpf_grid, values_host, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's array is free again
  for (int a = 0; a < 3; a++) {
    c->gpf_par.origin[a] = origin[a];
    c->gpf_par.dims[a] = dims[a];
  }
  c->gpf_par.resolution = resolution;
  c->gpf_par.unknown_loglike = unknown_loglike;
  c->gpf_par.cov_scaling = cov_scaling;
  c->gpf_grid_on = true;
  return PB_OK;
}

extern "C" int pb_gpf_grid_loglik(pb_ctx *c, int K, const double *pose_dev, int n_points, const double *points, int points_mem,
                                  double *loglik_out_dev)
{
  CALL(c, NEEDS_STATE);
  if (!c->gpf_grid_on) return fail(c, PB_ERR_ARG, "pb_gpf_grid_loglik before pb_gpf_grid_set");
  if (K < 1 || n_points < 0) return fail(c, PB_ERR_ARG, "pb_gpf_grid_loglik: K must be at least 1 and n_points at least 0 (got %d, %d)", K, n_points);
  if (!pose_dev || !loglik_out_dev || (n_points > 0 && !points)) return fail(c, PB_ERR_ARG, "pb_gpf_grid_loglik: NULL block");
  const double *pts = points;
  if (n_points > 0 && points_mem == PB_HOST_BROADCAST) {
    const size_t n = 3 * (size_t) n_points;
    if (n > c->gpf_pts_n) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      c->gpf_pts_n = 0;
      HIPCHK(c, dev_release(c, c->gpf_pts));
      if (int rc = dev_alloc(c, c->gpf_pts, n)) return rc;
      c->gpf_pts_n = n;
    }
    HIPCHK(c, hipMemcpyAsync(c->gpf_pts, points, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    pts = c->gpf_pts;
  } else if (n_points > 0) {
    Part p[1] = { { points, sizeof(double) * 3 * (size_t) n_points * (size_t) c->B, 0 } };
    if (int rc = stage_in(c, points_mem, p, 1)) return rc;
    pts = (const double *) p[0].dev;
  }
  k_gpf_grid_loglik<<<dim3(nblk(c->B), std::min(K, 65535)), 64, 0, c->stream>>>(c->gpf_par, c->gpf_grid, c->B, K, pose_dev, n_points, pts,
                                                                                 points_mem == PB_HOST_BROADCAST, loglik_out_dev);
  LAUNCHCHK(c);
  return PB_OK;
}
