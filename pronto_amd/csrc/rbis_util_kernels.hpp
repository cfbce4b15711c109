// rbis_util_kernels.hpp -- the small kernels around the filter: reset, read-back, snapshot / compose, summary, broadcast fill, the
// noise-identification window likelihood and the counter-calibration copy.  Launched from pronto_batch.hip only, and included by it
// only: k_compose, k_fill_rows and k_calib_copy are plain (non-template) kernels, emitted by every object that sees them.
#pragma once

#include "rbis_tile_io.hpp"

namespace pb {

// RBISResetUpdate::updateFilter, per-filter inputs: vec [n][B], quat [4][B], cov [n*n][B] column-major
template <int NS>
__global__ void k_reset(double *__restrict__ st, int B, const double *__restrict__ vec,
                        const double *__restrict__ quat, const double *__restrict__ cov, const double *__restrict__ ll = nullptr)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < NS; i++) st[S::eidx(L::OFF_VEC + i, b)] = vec[(long) i * B + b];
  for (int i = 0; i < 4; i++) st[S::eidx(L::OFF_QUAT + i, b)] = quat[(long) i * B + b];
  st[S::eidx(L::OFF_LL, b)] = ll ? ll[b] : 0.0;
  for (int i = 0; i < NS; i++)
    for (int j = 0; j <= i; j++) st[S::eidx(L::OFF_P + pk(i, j), b)] = cov[(long) (j * NS + i) * B + b];
}

// broadcast reset: comp [NC] in canonical component order, packed on the host
template <int NS>
__global__ void k_reset_bcast(double *__restrict__ st, int B, const double *__restrict__ comp)
{
  using S = Slots<NS>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int c = 0; c < Lay<NS>::NC; c++) st[S::eidx(c, b)] = comp[c];
}

template <int NS>
__global__ void k_get_head(const double *__restrict__ st, int first, int count, double *vec_out,
                           double *quat_out, double *cov_out, double *ll_out)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int b = first + t;
  if (vec_out)
    for (int i = 0; i < NS; i++) vec_out[(long) i * count + t] = st[S::eidx(L::OFF_VEC + i, b)];
  if (quat_out)
    for (int i = 0; i < 4; i++) quat_out[(long) i * count + t] = st[S::eidx(L::OFF_QUAT + i, b)];
  if (ll_out) ll_out[t] = st[S::eidx(L::OFF_LL, b)];
  if (cov_out)
    for (int c = 0; c < NS; c++)
      for (int r = 0; r < NS; r++)
        cov_out[(long) (c * NS + r) * count + t] = st[S::eidx(L::OFF_P + pk(r, c), b)];
}

// (position, quat) of the head posterior -> snapshot slot [7][stride]
template <int NS>
__global__ void k_snapshot(const double *__restrict__ st, long stride, int B, double *__restrict__ snap)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < 3; i++) snap[(long) i * stride + b] = st[S::eidx(L::OFF_VEC + 9 + i, b)];
  for (int i = 0; i < 4; i++) snap[(long) (3 + i) * stride + b] = st[S::eidx(L::OFF_QUAT + i, b)];
}

// T1 = T0 * (t, q)   (rbis_fovis_update.cpp:219-223)
static __global__ void k_compose(const double *__restrict__ snap, long stride, int B, const double *__restrict__ t,
                          const double *__restrict__ q, double *__restrict__ z_out, double *__restrict__ q_out)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double p0[3] = { snap[b], snap[stride + b], snap[2 * stride + b] };
  const double q0[4] = { snap[3 * stride + b], snap[4 * stride + b], snap[5 * stride + b], snap[6 * stride + b] };
  const double tt[3] = { t[b], t[(long) B + b], t[2L * B + b] };
  const double qq[4] = { q[b], q[(long) B + b], q[2L * B + b], q[3L * B + b] };
  double R[9], o[4];
  quat_to_rot(q0, R);
  for (int i = 0; i < 3; i++)
    z_out[(long) i * B + b] = p0[i] + (R[3 * i] * tt[0] + R[3 * i + 1] * tt[1] + R[3 * i + 2] * tt[2]);
  quat_mul(q0, qq, o);
  for (int i = 0; i < 4; i++) q_out[(long) i * B + b] = o[i];
}

template <int NS>
__global__ void k_summary(const double *__restrict__ st, int B, double *__restrict__ out)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  double s_ll = 0, s_abs = 0, qdev = 0, nonfin = 0;
  if (b < B) {
    s_ll = st[S::eidx(L::OFF_LL, b)];
    double qn = 0;
    for (int i = 0; i < NS + 4; i++) {
      const double v = st[S::eidx(i, b)];
      s_abs += fabs(v);
      if (!isfinite(v)) nonfin += 1;
      if (i >= NS) qn += v * v;
    }
    for (int i = 0; i < L::NP; i++)
      if (!isfinite(st[S::eidx(L::OFF_P + i, b)])) nonfin += 1;
    if (!isfinite(s_ll)) nonfin += 1;
    qdev = fabs(qn - 1.0);
  }
  for (int off = 32; off > 0; off >>= 1) {
    s_ll += __shfl_down(s_ll, off);
    s_abs += __shfl_down(s_abs, off);
    nonfin += __shfl_down(nonfin, off);
    qdev = fmax(qdev, __shfl_down(qdev, off));
  }
  // one partial per wave, reduced on the host in wave order: bit-reproducible (float atomics are not)
  if ((threadIdx.x & 63) == 0) {
    double *o = out + 4L * blockIdx.x;
    o[0] = s_ll; o[1] = s_abs; o[2] = qdev; o[3] = nonfin;
  }
}

static __global__ void k_fill_rows(double *__restrict__ dst, int rows, int B, RowVals vals)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int r = 0; r < rows; r++) dst[(long) r * B + b] = vals.v[r];
}

// Noise identification (state-estimator/src/noise_id/noise_id.cpp:37-38,44-65): window error e = head (-) truth with
// chi = Log(truth.quat^-1 * quat), then over the m active indices log det P_aa and e_a^T P_aa^-1 e_a (the two pieces of
// eigen_utils' loglike_normalized).  out [3][B] = logdet, mahalanobis^2, -0.5*(m log 2pi + logdet + maha).
// err_out [NS][B] (optional) receives the full error vector.  Runtime index list, gathered like k_update.
template <int NS, int M>
__global__ void k_window_nll(const double *__restrict__ st, int B, IdxArg<M> idx,
                             const double *__restrict__ tvec, const double *__restrict__ tquat, double *__restrict__ out,
                             double *__restrict__ err_out)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double q[4], tq[4], dchi[3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    q[i] = st[S::eidx(L::OFF_QUAT + i, b)];
    tq[i] = tquat[(long) i * B + b];
  }
  subtract_quats(q, tq, dchi);
  if (err_out != nullptr) {
    for (int i = 0; i < NS; i++) {
      double e = st[S::eidx(L::OFF_VEC + i, b)] - tvec[(long) i * B + b];
      if (i >= 6 && i <= 8) e = dchi[i - 6];
      err_out[(long) i * B + b] = e;
    }
  }
  double e[M], Sm[M * (M + 1) / 2], d[M];
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    const int ii = idx.v[kk];
    double v = st[S::eidx(L::OFF_VEC + ii, b)] - tvec[(long) ii * B + b];
    if (ii >= 6 && ii <= 8) v = (ii == 6) ? dchi[0] : (ii == 7 ? dchi[1] : dchi[2]);
    e[kk] = v;
#pragma unroll
    for (int j = 0; j <= kk; j++) Sm[pk(kk, j)] = st[S::eidx(L::OFF_P + pk(ii, idx.v[j]), b)];
  }
  ldlt<M>(Sm, d);
  double det = 1.0, maha = 0.0, y[M];
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    double s = e[kk];
#pragma unroll
    for (int j = 0; j < kk; j++) s -= Sm[pk(kk, j)] * y[j];
    y[kk] = s;
    det *= d[kk];
    maha += s * s / d[kk];
  }
  const double logdet = log(det);
  out[b] = logdet;
  out[(long) B + b] = maha;
  out[2L * B + b] = -0.5 * (M * 1.8378770664093453 + logdet + maha);  // log(2 pi)
}

// Counter calibration: a plain copy with EXACTLY the access pattern of the step kernels (buffer_load/store_dwordx4,
// 16 bytes per lane, one tile per wave, all loads of a chunk before its stores), so that rocprofv3's FETCH_SIZE /
// WRITE_SIZE can be scaled on a known byte count, and the copy ceiling of this access pattern measured.
static __global__ __launch_bounds__(64, 1) void k_calib_copy(const double *__restrict__ src, double *__restrict__ dst, int B,
                                                      int nrow)
{
  const unsigned tile = blockIdx.x;
  if (tile * 64u >= (unsigned) B) return;
  const unsigned tb = (unsigned) nrow * 1024u;
  const rsrc_t ri = mkbuf(reinterpret_cast<const char *>(src) + (size_t) tile * tb, tb);
  const rsrc_t ro = mkbuf(reinterpret_cast<char *>(dst) + (size_t) tile * tb, tb);
  const unsigned vo = threadIdx.x * 16u;
  for (int r0 = 0; r0 < nrow; r0 += 35) {
    d2_t v[35];
#pragma unroll
    for (int i = 0; i < 35; i++) v[i] = (r0 + i < nrow) ? ldg2(ri, (unsigned) (r0 + i) * 1024u, vo) : d2_t{ 0, 0 };
#pragma unroll
    for (int i = 0; i < 35; i++)
      if (r0 + i < nrow) stg2(ro, (unsigned) (r0 + i) * 1024u, vo, v[i]);
  }
}

}  // namespace pb
