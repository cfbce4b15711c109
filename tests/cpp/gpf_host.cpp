// gpf_host.cpp -- the per-lane functions of the GPF measurement (pronto_amd/csrc/rbis_gpf.hpp) compiled by g++: the same text the
// kernels of rbis_gpf_kernels.hpp run, over plain [rows][B] arrays.  Built as a shared object for tests/test_gpf_host.py, and with
// -DGPF_HOST_MAIN as a stand-alone program that runs a fixed batch (for -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pronto_amd/csrc/rbis_gpf.hpp"

using namespace pb;

template <int M>
static void sample_m(const int *idx, int K, int B, const double *Sig, const double *x6, const double *q, const double *xi, double tol,
                     double *delta, double *pose)
{
  int id[M];
  for (int i = 0; i < M; i++) id[i] = idx[i];
  for (int b = 0; b < B; b++) {
    double L[M * (M + 1) / 2], xx[6], qq[4];
    for (int i = 0; i < M; i++)
      for (int j = 0; j <= i; j++) L[pk(i, j)] = Sig[((size_t) i * M + j) * B + b];
    for (int i = 0; i < 6; i++) xx[i] = x6[(size_t) i * B + b];
    for (int i = 0; i < 4; i++) qq[i] = q[(size_t) i * B + b];
    const bool ok = gpf_chol<M>(L);
    for (int k = 0; k < K; k++) {
      double x[M], s[M], p[7];
      for (int i = 0; i < M; i++) x[i] = xi[((size_t) k * M + i) * B + b];
      gpf_sample<M>(L, ok, x, s);
      gpf_pose<M>(id, xx, qq, s, tol, p);
      for (int i = 0; i < M; i++) delta[((size_t) k * M + i) * B + b] = s[i];
      for (int i = 0; i < 7; i++) pose[((size_t) k * 7 + i) * B + b] = p[i];
    }
  }
}

// the fit as k_gpf_fit runs it: four fixed quarters, combined 0 + 1 + 2 + 3
template <int M>
static void fit_m(int K, int B, const double *Sig, const double *xm, const double *delta, const double *ll, double mwp, double *z, double *R,
                  int32_t *status)
{
  for (int b = 0; b < B; b++) {
    double mx = -INFINITY;
    bool bad = false;
    for (int k = 0; k < K; k++) {
      const double l = ll[(size_t) k * B + b];
      bad = bad || !(std::fabs(l) <= 1.7976931348623157e308);
      mx = l > mx ? l : mx;
    }
    GpfAcc<M> acc[4];
    for (int w = 0; w < 4; w++) {
      int first, last;
      gpf_quarter(K, w, first, last);
      acc[w].zero();
      for (int k = first; k < last; k++) {
        double s[M];
        for (int i = 0; i < M; i++) s[i] = delta[((size_t) k * M + i) * B + b];
        acc[w].add(s, std::exp(ll[(size_t) k * B + b] - mx));
      }
    }
    for (int w = 1; w < 4; w++) acc[0].merge(acc[w]);
    double zz[M], RR[M * M];
    const int st = gpf_fit_solve<M>(
        acc[0], K, mwp, bad,
        [&](double (&S)[M * (M + 1) / 2], double (&x)[M]) {
          for (int i = 0; i < M; i++) {
            x[i] = xm[(size_t) i * B + b];
            for (int j = 0; j <= i; j++) S[pk(i, j)] = Sig[((size_t) i * M + j) * B + b];
          }
        },
        zz, RR);
    for (int i = 0; i < M; i++) z[(size_t) i * B + b] = zz[i];
    for (int i = 0; i < M * M; i++) R[(size_t) i * B + b] = RR[i];
    status[b] = st;
  }
}

#define GPF_M_CASES(CALL) \
  switch (m) {            \
  case 1: CALL(1); break; \
  case 2: CALL(2); break; \
  case 3: CALL(3); break; \
  case 4: CALL(4); break; \
  case 5: CALL(5); break; \
  case 6: CALL(6); break; \
  case 7: CALL(7); break; \
  case 8: CALL(8); break; \
  case 9: CALL(9); break; \
  default: return 1;      \
  }

extern "C" {
void gpf_host_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
  const Philox4 p = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int i = 0; i < 4; i++) out[i] = p.w[i];
}
void gpf_host_normals(uint64_t seed, uint32_t stream_id, int rows, int B, double *out)
{
  for (int b = 0; b < B; b++)
    for (int j = 0; 2 * j < rows; j++) {
      double n0, n1;
      gpf_normal_pair(seed, stream_id, (uint32_t) b, (uint32_t) j, n0, n1);
      out[(size_t) (2 * j) * B + b] = n0;
      if (2 * j + 1 < rows) out[(size_t) (2 * j + 1) * B + b] = n1;
    }
}
// Sig [m][m][B] (the lower triangle is read), x6 [6][B] = vec[6..11], q [4][B], xi [K][m][B] -> delta [K][m][B], pose [K][7][B]
int gpf_host_sample(int m, const int *idx, int K, int B, const double *Sig, const double *x6, const double *q, const double *xi, double tol,
                    double *delta, double *pose)
{
#define CALL(M) sample_m<M>(idx, K, B, Sig, x6, q, xi, tol, delta, pose)
  GPF_M_CASES(CALL)
#undef CALL
  return 0;
}
// xm [m][B] = x[idx], delta [K][m][B], ll [K][B] -> z [m][B], R [m*m][B] column-major, status [B]
int gpf_host_fit(int m, int K, int B, const double *Sig, const double *xm, const double *delta, const double *ll, double mwp, double *z, double *R,
                 int32_t *status)
{
#define CALL(M) fit_m<M>(K, B, Sig, xm, delta, ll, mwp, z, R, status)
  GPF_M_CASES(CALL)
#undef CALL
  return 0;
}
// values [nz][ny][nx]; one sample pose (7) and n points [3 n] -> the sum of the scores / cov_scaling
double gpf_host_grid(const double origin[3], double res, const int dims[3], const double *values, double unknown, double cov, const double pose[7],
                     int n, const double *pts)
{
  GpfGrid g;
  for (int a = 0; a < 3; a++) { g.origin[a] = origin[a]; g.dims[a] = dims[a]; }
  g.resolution = res; g.unknown_loglike = unknown; g.cov_scaling = cov;
  const double t[3] = { pose[0], pose[1], pose[2] }, q[4] = { pose[3], pose[4], pose[5], pose[6] };
  double Rm[9], sum = 0.0;
  quat_to_rot(q, Rm);
  for (int p = 0; p < n; p++) {
    if (!(std::fabs(pts[3 * p]) <= 1.7976931348623157e308)) continue;
    sum += gpf_grid_point(g, Rm, t, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], [&](long i) { return values[i]; });
  }
  return sum / cov;
}
}

#ifdef GPF_HOST_MAIN
// a fixed batch through every M: diagonal-dominant Sigma_bar, Gaussian log-likelihoods, one flat and one NaN filter
int main()
{
  const int B = 5, K = 64;
  for (int m = 1; m <= 9; m++) {
    std::vector<int> idx(m);
    for (int i = 0; i < m; i++) idx[i] = 11 - i;
    std::vector<double> Sig((size_t) m * m * B), x6(6 * B, 0.25), q(4 * B, 0.0), xi((size_t) K * m * B), delta(xi.size()), pose((size_t) K * 7 * B),
        xm((size_t) m * B, 1.0), ll((size_t) K * B), z((size_t) m * B), R((size_t) m * m * B);
    std::vector<int32_t> status(B);
    for (int b = 0; b < B; b++) {
      q[b] = 1.0;
      for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) Sig[((size_t) i * m + j) * B + b] = (i == j ? 0.04 * (1 + i) : 0.002) * (b == 4 ? -1.0 : 1.0);
    }
    gpf_host_normals(12345u + m, 7u, K * m, B, xi.data());
    if (gpf_host_sample(m, idx.data(), K, B, Sig.data(), x6.data(), q.data(), xi.data(), 1e-6, delta.data(), pose.data())) return 2;
    for (int k = 0; k < K; k++)
      for (int b = 0; b < B; b++) {
        double s = 0.0;
        for (int i = 0; i < m; i++) {
          const double d = delta[((size_t) k * m + i) * B + b] - 0.05;
          s += d * d / (0.08 * (1 + i));
        }
        ll[(size_t) k * B + b] = b == 2 ? 0.0 : (b == 3 && k == 5 ? NAN : -0.5 * s);
      }
    if (gpf_host_fit(m, K, B, Sig.data(), xm.data(), delta.data(), ll.data(), 0.999, z.data(), R.data(), status.data())) return 3;
    if (status[2] != 2 || status[3] != 2 || status[4] != 2) return 4;
    for (int i = 0; i < m * B; i++)
      if (!(std::fabs(z[i]) < 1e300)) return 5;
  }
  const double origin[3] = { -1, -1, -1 }, pose[7] = { 0.1, 0.2, 0.3, 0.8, 0.2, -0.4, 0.4 }, pts[9] = { 0.5, 0.5, 0.5, NAN, 0, 0, 9, 9, 9 };
  const int dims[3] = { 4, 3, 2 };
  std::vector<double> values(24, -0.5);
  if (!(std::fabs(gpf_host_grid(origin, 1.0, dims, values.data(), -12.0, 2.0, pose, 3, pts)) < 100.0)) return 6;
  printf("ok\n");
  return 0;
}
#endif
