// rbis_gpf_kernels.hpp -- the kernels of the GPF measurement (rbis_gpf.hpp), launched from pb_gpf.hip only.  Lanes run along filters
// in every one of them: a wave's access to a [rows][B] block is 64 consecutive doubles.
//   k_gpf_normals      one thread per (filter, row pair): Philox4x32-10 + Box-Muller, no state
//   k_gpf_sample       blockIdx.y walks chunks of GPF_SAMPLE_CHUNK samples; each thread gathers Sigma_bar and factors it once
//                      (<= 165 flops, cheaper than a second kernel), then loops over its chunk
//   k_gpf_fit          one workgroup of four waves per tile of 64 filters (one wave per SIMD: the nine-row instance holds
//                      2 x (45 + 9) + 1 accumulators).  The waves take fixed quarters of the K samples and combine max l, then the
//                      sums, through LDS in the order 0 + 1 + 2 + 3: no atomics, the same bits from run to run.  The M x M algebra
//                      runs on wave 0's lanes.
//   k_gpf_grid_loglik  one thread per (filter, sample), a loop over the points; the grid and broadcast points come through the caches
// The index list is a kernel argument, the same for every lane: the host turns it into element offsets (GpfTab), so nothing is
// indexed at run time.
#pragma once

#include "rbis_gpf.hpp"

namespace pb {

constexpr int GPF_SAMPLE_CHUNK = 16;

// double offsets into a tile of lane 0's copy of a component (a lane adds 2 * lane)
template <int M>
struct GpfTab {
  unsigned blk[M * (M + 1) / 2];  // P(idx_k, idx_j), packed lower
  unsigned xm[M];                 // x[idx_k]
  int idx[M];
};
template <int NS>
constexpr unsigned gpf_offset(int comp)
{
  const int sl = Slots<NS>::T.slot_of[comp];
  return (unsigned) (sl >> 1) * 128u + (unsigned) (sl & 1);
}
template <int NS, int M>
inline GpfTab<M> make_gpf_tab(const int *idx)
{
  using L = Lay<NS>;
  GpfTab<M> t;
  for (int k = 0; k < M; k++) {
    t.idx[k] = idx[k];
    t.xm[k] = gpf_offset<NS>(L::OFF_VEC + idx[k]);
    for (int j = 0; j <= k; j++) t.blk[pk(k, j)] = gpf_offset<NS>(L::OFF_P + pk(idx[k], idx[j]));
  }
  return t;
}

// out [rows][B]; grid (tiles, row pairs)
__global__ __launch_bounds__(64) void k_gpf_normals(uint64_t seed, uint32_t stream_id, int rows, int B, double *__restrict__ out)
{
  const unsigned b = blockIdx.x * 64u + threadIdx.x;
  if (b >= (unsigned) B) return;
  for (unsigned j = blockIdx.y; 2u * j < (unsigned) rows; j += gridDim.y) {
    double n0, n1;
    gpf_normal_pair(seed, stream_id, b, j, n0, n1);
    out[(size_t) (2u * j) * B + b] = n0;
    if (2u * j + 1u < (unsigned) rows) out[(size_t) (2u * j + 1u) * B + b] = n1;
  }
}

// xi, delta [K][M][B]; pose [K][7][B]; grid (tiles, chunks of samples)
template <int NS, int M>
__global__ __launch_bounds__(64) void k_gpf_sample(const double *__restrict__ st, int B, GpfTab<M> tab, int K, const double *__restrict__ xi,
                                                   double *__restrict__ delta, double *__restrict__ pose, double chi_tol)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const unsigned lane = threadIdx.x, b = blockIdx.x * 64u + lane;
  if (b >= (unsigned) B) return;
  const double *tl = st + (size_t) blockIdx.x * S::TILE_DOUBLES + 2u * lane;
  double Lc[M * (M + 1) / 2], x6[6], q[4];
#pragma unroll
  for (int i = 0; i < M * (M + 1) / 2; i++) Lc[i] = tl[tab.blk[i]];
#pragma unroll
  for (int i = 0; i < 6; i++) x6[i] = tl[gpf_offset<NS>(L::OFF_VEC + 6 + i)];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = tl[gpf_offset<NS>(L::OFF_QUAT + i)];
  const bool ok = gpf_chol<M>(Lc);
  const int k0 = blockIdx.y * GPF_SAMPLE_CHUNK, k1 = k0 + GPF_SAMPLE_CHUNK < K ? k0 + GPF_SAMPLE_CHUNK : K;
  for (int k = k0; k < k1; k++) {
    double x[M], s[M], p[7];
#pragma unroll
    for (int i = 0; i < M; i++) x[i] = xi[((size_t) k * M + i) * B + b];
    gpf_sample<M>(Lc, ok, x, s);
    gpf_pose<M>(tab.idx, x6, q, s, chi_tol, p);
#pragma unroll
    for (int i = 0; i < M; i++) delta[((size_t) k * M + i) * B + b] = s[i];
#pragma unroll
    for (int i = 0; i < 7; i++) pose[((size_t) k * 7 + i) * B + b] = p[i];
  }
}

// delta [K][M][B], ll [K][B] -> z [M][B], R [M * M][B], status [B]; grid (tiles), 256 threads
template <int NS, int M>
__global__ __launch_bounds__(256) void k_gpf_fit(const double *__restrict__ st, int B, GpfTab<M> tab, int K, const double *__restrict__ delta,
                                                 const double *__restrict__ ll, double max_weight_proportion, double *__restrict__ z_out,
                                                 double *__restrict__ R_out, int32_t *__restrict__ status_out)
{
  using S = Slots<NS>;
  using Acc = GpfAcc<M>;
  __shared__ double red[Acc::N][64];
  __shared__ double mx[4][64];
  __shared__ int nf[4][64];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned b = blockIdx.x * 64u + lane;
  const bool live = b < (unsigned) B;
  const unsigned bc = live ? b : (unsigned) B - 1u;  // a lane past the batch reads the last filter and stores nothing: every lane meets every barrier
  int first, last;
  gpf_quarter(K, (int) wave, first, last);
  // max l of the quarter; a quarter without samples contributes -inf
  double m = -__builtin_inf();
  int bad = 0;
  for (int k = first; k < last; k++) {
    const double l = ll[(size_t) k * B + bc];
    bad |= !(fabs(l) <= 1.7976931348623157e308);
    m = l > m ? l : m;
  }
  mx[wave][lane] = m;
  nf[wave][lane] = bad;
  __syncthreads();
  m = mx[0][lane];
  bad = nf[0][lane];
#pragma unroll
  for (int w = 1; w < 4; w++) {
    m = mx[w][lane] > m ? mx[w][lane] : m;
    bad |= nf[w][lane];
  }
  Acc acc;
  acc.zero();
  for (int k = first; k < last; k++) {
    double s[M];
#pragma unroll
    for (int i = 0; i < M; i++) s[i] = delta[((size_t) k * M + i) * B + bc];
    acc.add(s, exp(ll[(size_t) k * B + bc] - m));
  }
  // wave 0 += wave 1, += wave 2, += wave 3, entry by entry through one LDS block
  for (unsigned w = 1; w < 4; w++) {
    if (wave == w) {
      red[0][lane] = acc.W;
#pragma unroll
      for (int i = 0; i < M; i++) { red[1 + i][lane] = acc.sw[i]; red[1 + M + i][lane] = acc.su[i]; }
#pragma unroll
      for (int i = 0; i < Acc::NP; i++) { red[1 + 2 * M + i][lane] = acc.sww[i]; red[1 + 2 * M + Acc::NP + i][lane] = acc.suu[i]; }
    }
    __syncthreads();
    if (wave == 0) {
      Acc o;
      o.W = red[0][lane];
#pragma unroll
      for (int i = 0; i < M; i++) { o.sw[i] = red[1 + i][lane]; o.su[i] = red[1 + M + i][lane]; }
#pragma unroll
      for (int i = 0; i < Acc::NP; i++) { o.sww[i] = red[1 + 2 * M + i][lane]; o.suu[i] = red[1 + 2 * M + Acc::NP + i][lane]; }
      acc.merge(o);
    }
    __syncthreads();
  }
  if (wave != 0 || !live) return;
  const double *tl = st + (size_t) blockIdx.x * S::TILE_DOUBLES + 2u * lane;
  double z[M], R[M * M];
  const int status = gpf_fit_solve<M>(
      acc, K, max_weight_proportion, bad != 0,
      [&](double (&Sig)[M * (M + 1) / 2], double (&xm)[M]) {
#pragma unroll
        for (int i = 0; i < M * (M + 1) / 2; i++) Sig[i] = tl[tab.blk[i]];
#pragma unroll
        for (int i = 0; i < M; i++) xm[i] = tl[tab.xm[i]];
      },
      z, R);
#pragma unroll
  for (int i = 0; i < M; i++) z_out[(size_t) i * B + b] = z[i];
#pragma unroll
  for (int i = 0; i < M * M; i++) R_out[(size_t) i * B + b] = R[i];
  status_out[b] = status;
}

// pose [K][7][B]; points [3 n][B] (bcast 0) or [3 n] (bcast 1); out [K][B]; grid (tiles, samples)
__global__ __launch_bounds__(64) void k_gpf_grid_loglik(GpfGrid g, const double *__restrict__ values, int B, int K, const double *__restrict__ pose,
                                                        int n_points, const double *__restrict__ points, int bcast, double *__restrict__ out)
{
  const unsigned b = blockIdx.x * 64u + threadIdx.x;
  if (b >= (unsigned) B) return;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    double t[3], q[4], Rm[9];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = pose[((size_t) k * 7 + i) * B + b];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = pose[((size_t) k * 7 + 3 + i) * B + b];
    quat_to_rot(q, Rm);
    double sum = 0.0;
    for (int p = 0; p < n_points; p++) {
      double px, py, pz;
      if (bcast) {
        px = points[3 * p]; py = points[3 * p + 1]; pz = points[3 * p + 2];
      } else {
        px = points[(size_t) (3 * p) * B + b]; py = points[(size_t) (3 * p + 1) * B + b]; pz = points[(size_t) (3 * p + 2) * B + b];
      }
      if (!(fabs(px) <= 1.7976931348623157e308)) continue;  // stands in for the reference's point_status filter
      sum += gpf_grid_point(g, Rm, t, px, py, pz, [&](long i) { return values[i]; });
    }
    out[(size_t) k * B + b] = sum / g.cov_scaling;
  }
}

}  // namespace pb
