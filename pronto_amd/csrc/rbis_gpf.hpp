// rbis_gpf.hpp -- the Gaussian particle filter measurement (state-estimator/src/gpf/gpf.hpp:53-192, its twin under
// motion_estimate/src/gpf-rgbd-lib/, rbis_gpf_update.cpp:28-76) as per-lane arithmetic: everything here is a PB_HD function templated on
// the number of measured rows M, compiled by hipcc for the kernels of rbis_gpf_kernels.hpp and by g++ for tests/cpp/gpf_host.cpp.
//
// Per filter, with the index list idx of M rows and K samples:
//   gpf.hpp:68-81    Sigma_bar = P[idx, idx], L its lower Cholesky factor                       gpf_chol
//   gpf.hpp:92-103   s_k = L xi_k; sample state = head with vec[idx_i] += s_k[i], then addState's fold of chi into the quaternion
//                    (dstate_samp is built by assignment to .vec, so its own quaternion is the identity)       gpf_sample, gpf_pose
//   gpf.hpp:106-118  w_k = exp(l_k - max l), W = sum w_k; the fit runs only if 5 M < W < max_weight_proportion K, both strict
//   gpf.hpp:120-159  (mu_u, C_u), (mu_w, C_w) = fitParticles with unit weights / with w; R_eff = (C_w^-1 - C_u^-1)^-1;
//                    S = Sigma_bar + R_eff; K_eff^T = S^-1 C_u; z_eff = x[idx] + K_eff^-1 (mu_w - mu_u)
//   gpf.hpp:164-190  eigenvalues of R_eff below zero are set to 1e4, R_eff = V Lambda V^T                       gpf_fit_solve
//   gpf.hpp:193-200  otherwise R_eff = 1e4 I, z_eff = x[idx]
//
// fitParticles is eigen_utils', which is not in the reference tree.  Assumed semantics (as SURVEY 8a does for its siblings):
//   mean = sum w_k x_k / sum w_k;  cov = sum w_k (x_k - mean)(x_k - mean)^T / sum w_k, with no (K - 1) correction.
// The sums are kept as raw moments about zero (GpfAcc): the samples are deltas about the head, so the mean is a fraction of the spread.
//
// How the algebra is done (the reference: partial-pivot LU inverses, a pivoted LDL^T solve and a column-pivoted QR solve):
//   C_u and C_w are positive definite: inverted through their Cholesky factors.
//   D = C_w^-1 - C_u^-1 is symmetric and may be indefinite.  ONE cyclic Jacobi sweep loop gives D = V diag(lam) V^T; then
//   R_eff = V diag(1 / lam) V^T, its eigenvalues are 1 / lam (negative where lam is), and the repair replaces 1 / lam by 1e4 there.
//   K_eff = C_u S^-1 (both symmetric), so K_eff^-1 (mu_w - mu_u) = S C_u^-1 (mu_w - mu_u) = (Sigma_bar + R_eff) t with t = C_u^-1 (mu_w - mu_u):
//   no solve with the indefinite S is left, and z_eff uses the unrepaired 1 / lam as the reference does.
// Status: 0 as computed, 1 repaired, 2 the weight-sum branch.  Also status 2 (the reference has no such case: it would divide by zero
// or carry NaN): a non-finite log-likelihood, or a C_u / C_w that is not positive definite (all samples equal: the sampler's answer to a
// Sigma_bar that is not positive definite).
//
// All loops have compile-time bounds: every array index is a constant, the arrays stay in registers.
#pragma once

#include <cstdint>

#include "rbis_device.hpp"

namespace pb {

constexpr int GPF_MAX_ROWS = 9;
constexpr double GPF_R_NEG_EIG_CORRECTION = 1e4;  // gpf.hpp:14
constexpr int GPF_JACOBI_SWEEPS = 16;             // cap; the loop ends when the off-diagonal part is below 1e-17 of the diagonal

// ---- counter-based normals: Philox4x32-10 (Salmon et al., SC'11), Box-Muller ----
struct Philox4 {
  uint32_t w[4];
};
PB_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t) p1, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t) p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{ { c0, c1, c2, c3 } };
}
// a uniform in (0, 1) from two words: ((hi 2^32 + lo) >> 11 + 0.5) 2^-53
PB_HD double gpf_uniform(uint32_t hi, uint32_t lo)
{
  const uint64_t x = (((uint64_t) hi << 32) | lo) >> 11;
  return ((double) x + 0.5) * 1.1102230246251565e-16;
}
// the two normals of (filter b, row pair j) of stream stream_id: rows 2j and 2j + 1
PB_HD void gpf_normal_pair(uint64_t seed, uint32_t stream_id, uint32_t b, uint32_t j, double &n0, double &n1)
{
  const Philox4 p = philox4x32_10(b, j, stream_id, 0u, (uint32_t) seed, (uint32_t) (seed >> 32));
  const double u1 = gpf_uniform(p.w[0], p.w[1]), u2 = gpf_uniform(p.w[2], p.w[3]);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
  n0 = r * cos(a);
  n1 = r * sin(a);
}

// ---- sampling ----
// A (packed lower) <- its lower Cholesky factor; false (A is left half done) when a pivot is not positive
template <int M>
PB_HD bool gpf_chol(double (&A)[M * (M + 1) / 2])
{
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; j++) {
    double d = A[pk(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) d = fma(-A[pk(j, k)], A[pk(j, k)], d);
    ok = ok && (d > 0.0) && (d < 1.7976931348623157e308);
    const double l = sqrt(d), il = 1.0 / l;
    A[pk(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < M; i++) {
      double s = A[pk(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s = fma(-A[pk(i, k)], A[pk(j, k)], s);
      A[pk(i, j)] = s * il;
    }
  }
  return ok;
}
// s = L xi (ok), or 0 (the filter's Sigma_bar is not positive definite: every sample is the head)
template <int M>
PB_HD void gpf_sample(const double (&L)[M * (M + 1) / 2], bool ok, const double (&xi)[M], double (&s)[M])
{
#pragma unroll
  for (int i = 0; i < M; i++) {
    double a = L[pk(i, 0)] * xi[0];
#pragma unroll
    for (int j = 1; j <= i; j++) a = fma(L[pk(i, j)], xi[j], a);
    s[i] = ok ? a : 0.0;
  }
}
// The pose of the sample state: x6 = head vec[6..11] (chi, position), q the head quaternion; out = position xyz, quaternion wxyz
// (RBIS::getBotTrans).  idx is the same for every lane: selects, not indexed writes.
template <int M>
PB_HD void gpf_pose(const int (&idx)[M], const double (&x6)[6], const double (&q)[4], const double (&s)[M], double chi_tol, double (&out)[7])
{
  double v[6], qq[4] = { q[0], q[1], q[2], q[3] };
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double a = x6[r];
#pragma unroll
    for (int i = 0; i < M; i++) a = (idx[i] == 6 + r) ? x6[r] + s[i] : a;
    v[r] = a;
  }
  double chi[3] = { v[0], v[1], v[2] };
  fold_chi(chi, qq, chi_tol);
  out[0] = v[3]; out[1] = v[4]; out[2] = v[5];
  out[3] = qq[0]; out[4] = qq[1]; out[5] = qq[2]; out[6] = qq[3];
}

// ---- the fit ----
// raw moments of a run of samples: weighted and unit-weight
template <int M>
struct GpfAcc {
  static constexpr int NP = M * (M + 1) / 2;
  static constexpr int N = 1 + 2 * (M + NP);  // doubles, in the order of get / set
  double W, sw[M], su[M], sww[NP], suu[NP];
  PB_HD void zero()
  {
    W = 0.0;
#pragma unroll
    for (int i = 0; i < M; i++) sw[i] = su[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; i++) sww[i] = suu[i] = 0.0;
  }
  PB_HD void add(const double (&s)[M], double w)
  {
    W += w;
#pragma unroll
    for (int i = 0; i < M; i++) {
      const double ws = w * s[i];
      sw[i] += ws;
      su[i] += s[i];
#pragma unroll
      for (int j = 0; j <= i; j++) {
        sww[pk(i, j)] = fma(ws, s[j], sww[pk(i, j)]);
        suu[pk(i, j)] = fma(s[i], s[j], suu[pk(i, j)]);
      }
    }
  }
  // this += o, entry by entry: the kernel combines its four waves with it in a fixed order
  PB_HD void merge(const GpfAcc &o)
  {
    W += o.W;
#pragma unroll
    for (int i = 0; i < M; i++) { sw[i] += o.sw[i]; su[i] += o.su[i]; }
#pragma unroll
    for (int i = 0; i < NP; i++) { sww[i] += o.sww[i]; suu[i] += o.suu[i]; }
  }
};

// the share of wave w (0..3) of K samples: [first, last), fixed quarters of ceil(K / 4)
PB_HD void gpf_quarter(int K, int w, int &first, int &last)
{
  const int q = (K + 3) / 4;
  first = w * q < K ? w * q : K;
  last = (w + 1) * q < K ? (w + 1) * q : K;
}

// A (packed lower, positive definite) <- A^-1; false when A is not positive definite
template <int M>
PB_HD bool gpf_spd_inverse(double (&A)[M * (M + 1) / 2])
{
  const bool ok = gpf_chol<M>(A);
  // Li = L^-1 (lower), in place: column by column
  double Li[M * (M + 1) / 2];
#pragma unroll
  for (int j = 0; j < M; j++) {
    Li[pk(j, j)] = 1.0 / A[pk(j, j)];
#pragma unroll
    for (int i = j + 1; i < M; i++) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < i; k++) s = fma(A[pk(i, k)], Li[pk(k, j)], s);
      Li[pk(i, j)] = -s / A[pk(i, i)];
    }
  }
  // A^-1 = Li^T Li
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = i; k < M; k++) s = fma(Li[pk(k, i)], Li[pk(k, j)], s);
      A[pk(i, j)] = s;
    }
  return ok;
}

// A (packed lower, symmetric) = V diag(lam) V^T by cyclic Jacobi: A's diagonal becomes lam, V [row][column] the eigenvectors
template <int M>
PB_HD void gpf_jacobi(double (&A)[M * (M + 1) / 2], double (&V)[M][M])
{
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j < M; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  if constexpr (M > 1) {
    for (int sweep = 0; sweep < GPF_JACOBI_SWEEPS; sweep++) {
      double off = 0.0, dia = 0.0;
#pragma unroll
      for (int i = 0; i < M; i++) {
        dia = fma(A[pk(i, i)], A[pk(i, i)], dia);
#pragma unroll
        for (int j = 0; j < i; j++) off = fma(A[pk(i, j)], A[pk(i, j)], off);
      }
      if (!(off > 1e-34 * dia)) break;
#pragma unroll
      for (int p = 0; p < M - 1; p++)
#pragma unroll
        for (int q = p + 1; q < M; q++) {
          const double apq = A[pk(q, p)];
          // t = tan of the rotation angle, the smaller root; 0 when a_pq is 0 (theta is then inf or NaN)
          const double theta = (A[pk(q, q)] - A[pk(p, p)]) / (2.0 * apq);
          double t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
          t = theta < 0.0 ? -t : t;
          t = (apq != 0.0 && t == t) ? t : 0.0;
          const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
          A[pk(p, p)] = fma(-t, apq, A[pk(p, p)]);
          A[pk(q, q)] = fma(t, apq, A[pk(q, q)]);
          A[pk(q, p)] = 0.0;
#pragma unroll
          for (int k = 0; k < M; k++) {
            if (k != p && k != q) {
              const double akp = A[pk(k, p)], akq = A[pk(k, q)];
              A[pk(k, p)] = fma(c, akp, -s * akq);
              A[pk(k, q)] = fma(s, akp, c * akq);
            }
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = fma(c, vkp, -s * vkq);
            V[k][q] = fma(s, vkp, c * vkq);
          }
        }
    }
  }
}

// Steps 3-6 from the sums of all K samples.  bad: a log-likelihood of this filter was not finite.  ldprior(Sig, xm) fetches
// Sigma_bar = P[idx, idx] (packed lower) and x[idx] when they are needed, behind the eigen-decomposition (held from the start they cost
// 108 registers through it).  Out: z_eff [M], R_eff [M * M] column-major (symmetric).  -> status
template <int M, class LD>
PB_HD int gpf_fit_solve(const GpfAcc<M> &acc, int K, double max_weight_proportion, bool bad, LD ldprior, double (&z)[M], double (&R)[M * M])
{
  constexpr int NP = M * (M + 1) / 2;
  const double W = acc.W;
  bool fit = !bad && (5.0 * M < W) && (W < max_weight_proportion * (double) K);  // gpf.hpp:114-118
  double t[M], lam[M], V[M][M];
  {
    // fitParticles twice, then t = C_u^-1 (mu_w - mu_u) and D = C_w^-1 - C_u^-1.
    // (All of this also runs for a lane whose `fit` is false already -- W NaN or 0, a cloud that is not positive definite -- on NaN or
    // inf values: lanes do not branch apart, and the selects at the end discard the result.  The Jacobi loop ends there because its
    // test is written !(off > ...), which a NaN fails at the first sweep.)
    const double iw = 1.0 / W, iu = 1.0 / (double) K;
    double Cu[NP], Cw[NP], dm[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
      const double mwi = acc.sw[i] * iw, mui = acc.su[i] * iu;
      dm[i] = mwi - mui;
#pragma unroll
      for (int j = 0; j <= i; j++) {
        Cw[pk(i, j)] = fma(-mwi, acc.sw[j] * iw, acc.sww[pk(i, j)] * iw);
        Cu[pk(i, j)] = fma(-mui, acc.su[j] * iu, acc.suu[pk(i, j)] * iu);
      }
    }
    const bool oku = gpf_spd_inverse<M>(Cu), okw = gpf_spd_inverse<M>(Cw);
    fit = fit && oku && okw;
#pragma unroll
    for (int i = 0; i < M; i++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < M; j++) s = fma(Cu[pk(i, j)], dm[j], s);
      t[i] = s;
    }
#pragma unroll
    for (int i = 0; i < NP; i++) Cw[i] -= Cu[i];
    gpf_jacobi<M>(Cw, V);
#pragma unroll
    for (int i = 0; i < M; i++) lam[i] = Cw[pk(i, i)];
  }
  double Sig[NP], xm[M];
  ldprior(Sig, xm);
  // R_eff = V diag(1 / lam) V^T; z_eff from it as it is, R_eff itself with the eigenvalues below zero replaced (gpf.hpp:164-190)
  double rl[M], vt[M];
  bool repaired = false;
#pragma unroll
  for (int k = 0; k < M; k++) {
    const double il = 1.0 / lam[k];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < M; i++) s = fma(V[i][k], t[i], s);
    vt[k] = s * il;
    repaired = repaired || (il < 0.0);
    rl[k] = (il < 0.0) ? GPF_R_NEG_EIG_CORRECTION : il;
  }
#pragma unroll
  for (int i = 0; i < M; i++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < M; j++) s = fma(Sig[pk(i, j)], t[j], s);
#pragma unroll
    for (int k = 0; k < M; k++) s = fma(V[i][k], vt[k], s);
    z[i] = fit ? xm[i] + s : xm[i];
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double r = 0.0;
#pragma unroll
      for (int k = 0; k < M; k++) r = fma(V[i][k] * rl[k], V[j][k], r);
      r = fit ? r : (i == j ? GPF_R_NEG_EIG_CORRECTION : 0.0);
      R[j * M + i] = r;
      R[i * M + j] = r;
    }
  }
  return !fit ? 2 : (repaired ? 1 : 0);
}

// ---- the built-in likelihood: a dense voxel grid of -log-odds (LaserLikelihoodInterface.cpp:5-77 without octomap) ----
struct GpfGrid {
  double origin[3], resolution, unknown_loglike, cov_scaling;
  int dims[3];  // nx, ny, nz; values [nz][ny][nx]
};
// one point p (body frame) of the sample at position t with rotation Rm (row-major): its score
template <class VAL>
PB_HD double gpf_grid_point(const GpfGrid &g, const double (&Rm)[9], const double (&t)[3], double px, double py, double pz, VAL value)
{
  const double c[3] = { fma(Rm[0], px, fma(Rm[1], py, Rm[2] * pz)) + t[0], fma(Rm[3], px, fma(Rm[4], py, Rm[5] * pz)) + t[1],
                        fma(Rm[6], px, fma(Rm[7], py, Rm[8] * pz)) + t[2] };
  bool in = true;
  int v[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double u = (c[a] - g.origin[a]) / g.resolution;
    in = in && (c[a] >= g.origin[a]) && (c[a] <= g.origin[a] + g.dims[a] * g.resolution);
    const double f = floor(u);
    const int i = (f >= 0.0 && f < 2147483647.0) ? (int) f : 0;
    v[a] = i < g.dims[a] - 1 ? i : g.dims[a] - 1;
  }
  return in ? value(((long) v[2] * g.dims[1] + v[1]) * g.dims[0] + v[0]) : g.unknown_loglike;
}

}  // namespace pb
