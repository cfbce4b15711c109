// abi_recorder_gpf.cpp -- the recording stand-ins for the pb_gpf_* family, the C ABI functions pronto_amd/csrc/mav_state_est_gpf.hpp calls
// beyond those of mav_state_est_wide.hpp.  Linked beside the unchanged tests/cpp/abi_recorder.cpp and abi_recorder_wide.cpp; one line per
// call in that recorder's style: name, scalars, the index list in full, pointers by kind or checksum, never an address.
#include <cinttypes>
#include <cstdio>
#include <string>

#include "../../include/pronto_batch.h"
#include "abi_recorder.h"

// (the recorder's context, as tests/cpp/abi_recorder.cpp defines it)
struct pb_ctx {
  int n, B, nhist = 0;
  int out_slot = -1, pred_slot = -1, head_slot = -1;
  int gets = 0, fills = 0;
};

static std::string list_of(int m, const int *idx)
{
  std::string list = "[";
  for (int i = 0; i < m; i++) list += (i ? "," : "") + std::to_string(idx[i]);
  return list + "]";
}
static std::string dev(const void *p) { return rec_ptr(p, PB_DEVICE, 0); }

extern "C" int pb_gpf_normals(pb_ctx *, uint64_t seed, uint32_t stream_id, int rows, double *out)
{
  printf("pb_gpf_normals seed=%" PRIu64 " stream_id=%u rows=%d out=%s\n", seed, stream_id, rows, dev(out).c_str());
  return PB_OK;
}
extern "C" int pb_gpf_sample(pb_ctx *, int m, const int *idx, int K, const double *xi, double *delta, double *pose)
{
  printf("pb_gpf_sample m=%d idx=%s K=%d xi=%s delta=%s pose=%s\n", m, list_of(m, idx).c_str(), K, dev(xi).c_str(), dev(delta).c_str(), dev(pose).c_str());
  return PB_OK;
}
extern "C" int pb_gpf_measurement(pb_ctx *, int m, const int *idx, int K, const double *delta, const double *ll, double mwp, double *z, double *R,
                                  int32_t *status)
{
  printf("pb_gpf_measurement m=%d idx=%s K=%d delta=%s loglik=%s max_weight_proportion=%.17g z=%s R=%s status=%s\n", m, list_of(m, idx).c_str(), K,
         dev(delta).c_str(), dev(ll).c_str(), mwp, dev(z).c_str(), dev(R).c_str(), dev(status).c_str());
  return PB_OK;
}
extern "C" int pb_gpf_grid_set(pb_ctx *, const double origin[3], double resolution, const int dims[3], const double *values, double unknown_loglike,
                               double cov_scaling)
{
  printf("pb_gpf_grid_set origin=%s resolution=%.17g dims=[%d,%d,%d] values=%s unknown_loglike=%.17g cov_scaling=%.17g\n",
         rec_ptr(origin, PB_HOST, sizeof(double) * 3).c_str(), resolution, dims[0], dims[1], dims[2],
         rec_ptr(values, PB_HOST, sizeof(double) * (size_t) dims[0] * dims[1] * dims[2]).c_str(), unknown_loglike, cov_scaling);
  return PB_OK;
}
extern "C" int pb_gpf_grid_loglik(pb_ctx *c, int K, const double *pose, int n_points, const double *points, int points_mem, double *ll)
{
  const size_t per = points_mem == PB_HOST_BROADCAST ? 1 : (size_t) c->B;
  printf("pb_gpf_grid_loglik K=%d pose=%s n_points=%d points=%s points_mem=%d loglik=%s\n", K, dev(pose).c_str(), n_points,
         rec_ptr(points, points_mem, sizeof(double) * 3 * n_points * per).c_str(), points_mem, dev(ll).c_str());
  return PB_OK;
}
