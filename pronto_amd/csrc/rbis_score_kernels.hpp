// rbis_score_kernels.hpp -- the kernels of the ground-truth scorer (rbis_score.hpp).  Launched from pb_score.hip only, and included by
// it only.
//   k_score_gt<NS>      one lane per filter: on_pose_gt of drift_per_distance.py against the filter's position and quaternion
//   k_score_reset       pb_score_init's state
//   k_score_best_part / k_score_best_final   minimum and arg-min of a derived metric, two stages
#pragma once

#include "rbis_tile_io.hpp"
#include "rbis_score.hpp"

namespace pb {

// one ground-truth message: pose [7][B] on the device, or the seven values of one robot's truth for every filter
struct ScoreGt {
  const double *pose = nullptr;     // [7][B] pos[3], orientation[4]; NULL: bc
  double bc[7] = { 0, 0, 0, 1, 0, 0, 0 };
  const int64_t *utimes = nullptr;  // [B] or NULL: utime
  const uint8_t *valid = nullptr;   // [B] or NULL: every filter has the message
  int64_t utime = 0;
};

// The estimate is read through the slot map of the tiled state layout (Slots<NS>::eidx: position = vector rows 9..11, then the
// quaternion), from whichever array `st` the caller resolved.  No LDS, no atomics: a lane owns its filter's score state.  A filter
// without a message leaves after the read of its `valid` byte; lanes past B in the last tile leave at once.
template <int NS>
__global__ __launch_bounds__(64) void k_score_gt(const double *__restrict__ st, int B, long stride, ScorePar par, int flags, ScoreGt gt,
                                                 double *__restrict__ sd, int64_t *__restrict__ si)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const long b = (long) blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (gt.valid != nullptr && gt.valid[b] == 0) return;
  double p[3], q[4], ep[3], eq[4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    p[i] = gt.pose ? gt.pose[(long) i * B + b] : gt.bc[i];
    ep[i] = st[S::eidx(L::OFF_VEC + 9 + i, b)];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    q[i] = gt.pose ? gt.pose[(long) (3 + i) * B + b] : gt.bc[3 + i];
    eq[i] = st[S::eidx(L::OFF_QUAT + i, b)];
  }
  const int64_t t = gt.utimes ? gt.utimes[b] : gt.utime;
  score_message(sd, si, stride, b, par, flags, t, p, q, ep, eq);
}

__global__ __launch_bounds__(64) void k_score_reset(double *__restrict__ sd, int64_t *__restrict__ si, long stride)
{
  const long b = (long) blockIdx.x * 64 + threadIdx.x;
  if (b >= stride) return;
  score_reset(sd, si, stride, b);
}

// (value, filter) pairs ordered by value, then by filter index; filter < 0 = nothing yet
__device__ __forceinline__ void score_take_min(double &v, int &f, double ov, int of)
{
  if (of >= 0 && (f < 0 || ov < v || (ov == v && of < f))) {
    v = ov;
    f = of;
  }
}
__device__ __forceinline__ void score_wave_min(double &v, int &f)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int of = __shfl_xor(f, o);
    score_take_min(v, f, ov, of);
  }
}

constexpr int SCORE_BEST_PER_WG = 256;  // filters one 64-lane workgroup of the first stage covers (4 per lane)

// stage 1: workgroup w reduces the filters [w * SCORE_BEST_PER_WG, (w + 1) * SCORE_BEST_PER_WG) to one pair
__global__ __launch_bounds__(64) void k_score_best_part(const double *__restrict__ sd, const int64_t *__restrict__ si, long stride, int B,
                                                        int metric, double *__restrict__ part_v, int *__restrict__ part_f)
{
  double v = 0.0;
  int f = -1;
  const long b0 = (long) blockIdx.x * SCORE_BEST_PER_WG;
  for (int k = 0; k < SCORE_BEST_PER_WG / 64; k++) {
    const long b = b0 + (long) k * 64 + threadIdx.x;
    double m;
    if (b < B && score_metric(sd, si, stride, b, metric, m)) score_take_min(v, f, m, (int) b);
  }
  score_wave_min(v, f);
  if (threadIdx.x == 0) {
    part_v[blockIdx.x] = v;
    part_f[blockIdx.x] = f;
  }
}

// stage 2: one workgroup over the n_part pairs of stage 1; out_v[0], out_f[0]
__global__ __launch_bounds__(64) void k_score_best_final(const double *__restrict__ part_v, const int *__restrict__ part_f, int n_part,
                                                         double *__restrict__ out_v, int *__restrict__ out_f)
{
  double v = 0.0;
  int f = -1;
  for (int i = threadIdx.x; i < n_part; i += 64) score_take_min(v, f, part_v[i], part_f[i]);
  score_wave_min(v, f);
  if (threadIdx.x == 0) {
    out_v[0] = f >= 0 ? v : 0.0;
    out_f[0] = f;
  }
}

}  // namespace pb
