// wide_update_host.cpp -- TEST-ONLY: wide_update_lane (pronto_amd/csrc/rbis_update_wide.hpp), the per-lane arithmetic of k_update_wide,
// compiled with g++ over an in-memory tile: the glue below is the kernel's -- the gathers through the WideTab byte offsets, the row
// functors on 16-byte rows, the update in place -- with a plain array where the kernel keeps W in LDS.  tests/test_update_wide_host.py
// loads it as a shared library; with -DWIDE_HOST_MAIN it is a stand-alone program (its own main) for the sanitizer build.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pronto_batch.h"
#include "../../pronto_amd/csrc/rbis_update_wide.hpp"

using namespace pb;

namespace {

struct Pair {
  double x, y;
};

// R of filter b in the encoding rkind (enum pb_rkind) -> packed lower
template <int M>
void r_packed(const double *R, int rkind, int B, int b, double (&S)[M * (M + 1) / 2])
{
  for (int i = 0; i < M; i++)
    for (int j = 0; j <= i; j++) {
      if (rkind == PB_R_DIAG_BROADCAST) S[pk(i, j)] = (i == j) ? R[i] : 0.0;
      else if (rkind == PB_R_DIAG) S[pk(i, j)] = (i == j) ? R[(size_t) i * B + b] : 0.0;
      else S[pk(i, j)] = R[(size_t) (j * M + i) * B + b];
    }
}

// one update of every filter of a tiled state array, in place
template <int NS, int M, bool ORIENT>
void update_tiles(double *st, int B, const int *idx, const double *z, const double *R, int rkind, const double *qmeas, const uint8_t *mask,
                  const Consts &k)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  const WideTab<NS, M> tab = make_wide_tab<NS, M>(idx);
  for (int b = 0; b < B; b++) {
    if (mask && !mask[b]) continue;
    double *tile = st + (size_t) (b >> 6) * S::TILE_DOUBLES;
    const int lane = b & 63;
    auto at = [&](unsigned byte_off) -> double & { return tile[byte_off / 8 + 2 * lane]; };
    double zz[M], Sm[M * (M + 1) / 2], qm[4] = { 1.0, 0.0, 0.0, 0.0 }, q[4], xm[M];
    for (int i = 0; i < M; i++) zz[i] = z[(size_t) i * B + b];
    r_packed<M>(R, rkind, B, b, Sm);
    if (ORIENT)
      for (int i = 0; i < 4; i++) qm[i] = qmeas[(size_t) i * B + b];
    for (int i = 0; i < 4; i++) q[i] = at(wide_offset<NS>(L::OFF_QUAT + i));
    WideRegs<NS, M> W;
    for (int kk = 0; kk < M; kk++) {
      xm[kk] = at(tab.xm[kk]);
      for (int j = 0; j <= kk; j++) Sm[pk(kk, j)] += at(tab.blk[pk(kk, j)]);
    }
    for (int i = 0; i < NS; i++)
      for (int kk = 0; kk < M; kk++) W.set(i, kk, at(tab.col[i][kk]));
    wide_update_lane<NS, M, ORIENT>(
        tab.idx, q, xm, zz, qm, Sm, W,
        [&](double (&x)[NS], double &ll) {
          for (int i = 0; i < NS; i++) x[i] = at(wide_offset<NS>(L::OFF_VEC + i));
          ll = at(wide_offset<NS>(L::OFF_LL));
        },
        [&](int r) { return Pair{ tile[(size_t) r * 128 + 2 * lane], tile[(size_t) r * 128 + 2 * lane + 1] }; },
        [&](int r, double a, double c) {
          tile[(size_t) r * 128 + 2 * lane] = a;
          tile[(size_t) r * 128 + 2 * lane + 1] = c;
        },
        k);
  }
}

template <int NS>
int update_ns(double *st, int B, int m, const int *idx, const double *z, const double *R, int rkind, const double *qm, const uint8_t *mask,
              const Consts &k)
{
#define CASE(M)                                                                   \
  case M:                                                                         \
    if (qm) update_tiles<NS, M, true>(st, B, idx, z, R, rkind, qm, mask, k);      \
    else update_tiles<NS, M, false>(st, B, idx, z, R, rkind, qm, mask, k);        \
    return 0;
  switch (m) {
    CASE(7) CASE(8) CASE(9)
  }
#undef CASE
  return 1;
}

template <int NS>
void to_tiles(std::vector<double> &st, int B, const double *vec, const double *quat, const double *cov, const double *ll)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  st.assign((size_t) ((B + 63) / 64) * S::TILE_DOUBLES, 0.0);
  for (int b = 0; b < B; b++) {
    for (int i = 0; i < NS; i++) st[S::eidx(L::OFF_VEC + i, b)] = vec[(size_t) i * B + b];
    for (int i = 0; i < 4; i++) st[S::eidx(L::OFF_QUAT + i, b)] = quat[(size_t) i * B + b];
    st[S::eidx(L::OFF_LL, b)] = ll ? ll[b] : 0.0;
    for (int i = 0; i < NS; i++)
      for (int j = 0; j <= i; j++) st[S::eidx(L::OFF_P + pk(i, j), b)] = cov[(size_t) (j * NS + i) * B + b];
  }
}
template <int NS>
void from_tiles(const std::vector<double> &st, int B, double *vec, double *quat, double *cov, double *ll)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  for (int b = 0; b < B; b++) {
    for (int i = 0; i < NS; i++) vec[(size_t) i * B + b] = st[S::eidx(L::OFF_VEC + i, b)];
    for (int i = 0; i < 4; i++) quat[(size_t) i * B + b] = st[S::eidx(L::OFF_QUAT + i, b)];
    ll[b] = st[S::eidx(L::OFF_LL, b)];
    for (int i = 0; i < NS; i++)
      for (int j = 0; j < NS; j++) cov[(size_t) (j * NS + i) * B + b] = st[S::eidx(L::OFF_P + pk(i, j), b)];
  }
}

template <int NS>
int run(int B, int m, const int *idx, const double *z, const double *R, int rkind, const double *qm, const uint8_t *mask, double g, double tol,
        double *vec, double *quat, double *cov, double *ll)
{
  std::vector<double> st;
  to_tiles<NS>(st, B, vec, quat, cov, ll);
  const Consts k{ g, tol };
  if (int rc = update_ns<NS>(st.data(), B, m, idx, z, R, rkind, qm, mask, k)) return rc;
  from_tiles<NS>(st, B, vec, quat, cov, ll);
  return 0;
}

}  // namespace

// vec [n][B], quat [4][B], cov [n*n][B] column-major (the lower triangle is read; both triangles are written), ll [B]: the prior in, the
// posterior out.  z [m][B], R per rkind (enum pb_rkind), qm [4][B] or NULL, mask [B] or NULL.  Returns 0, or 1 for an m outside 7..9.
extern "C" int wide_host_update(int ns, int B, int m, const int *idx, const double *z, const double *R, int rkind, const double *qm,
                                const uint8_t *mask, double g, double tol, double *vec, double *quat, double *cov, double *ll)
{
  return ns == 15 ? run<15>(B, m, idx, z, R, rkind, qm, mask, g, tol, vec, quat, cov, ll)
                  : run<21>(B, m, idx, z, R, rkind, qm, mask, g, tol, vec, quat, cov, ll);
}

#ifdef WIDE_HOST_MAIN
// every instantiation once on 70 well-conditioned filters (a full tile and a six-lane tail), every second one masked off: finite
// posteriors, a smaller measured variance, masked filters untouched
int main()
{
  const int B = 70;
  int bad = 0;
  for (int ns : { 15, 21 })
    for (int m = 7; m <= 9; m++)
      for (int orient = 0; orient < 2; orient++)
        for (int rkind = 0; rkind < 3; rkind++) {
          int idx[9] = { 3, 4, 5, 6, 7, 8, 9, 10, 11 };
          if (m < 9) idx[0] = ns - 1;
          std::vector<double> vec((size_t) ns * B), quat(4 * (size_t) B), cov((size_t) ns * ns * B, 0.0), ll(B, 0.0), z((size_t) m * B), qm(4 * (size_t) B);
          std::vector<double> R(rkind == PB_R_FULL ? (size_t) m * m * B : (size_t) m * B, 0.0);
          std::vector<uint8_t> mask(B);
          for (int b = 0; b < B; b++) {
            mask[b] = b & 1;
            for (int i = 0; i < ns; i++) {
              vec[(size_t) i * B + b] = 0.01 * i + 0.001 * b;
              for (int j = 0; j < ns; j++) cov[(size_t) (j * ns + i) * B + b] = (i == j ? 0.5 + 0.01 * i : 0.0) + 0.02 / (1 + i + j);
            }
            vec[(size_t) 6 * B + b] = vec[(size_t) 7 * B + b] = vec[(size_t) 8 * B + b] = 0.0;
            quat[b] = 1.0;
            qm[b] = std::cos(0.05), qm[(size_t) B + b] = std::sin(0.05);
            for (int i = 0; i < m; i++) {
              z[(size_t) i * B + b] = vec[(size_t) idx[i] * B + b] + 0.1;
              if (rkind == PB_R_FULL) {
                for (int j = 0; j < m; j++) R[(size_t) (j * m + i) * B + b] = (i == j ? 0.2 : 0.01);
              } else if (rkind == PB_R_DIAG) R[(size_t) i * B + b] = 0.2;
              else R[i] = 0.2;
            }
          }
          const std::vector<double> v0 = vec, c0 = cov;
          if (wide_host_update(ns, B, m, idx, z.data(), R.data(), rkind, orient ? qm.data() : nullptr, mask.data(), 9.80665, 1e-6, vec.data(),
                               quat.data(), cov.data(), ll.data()))
            bad++;
          for (int b = 0; b < B; b++) {
            const size_t d = (size_t) (idx[1] * ns + idx[1]) * B + b;
            if (!mask[b] && (cov[d] != c0[d] || vec[(size_t) 3 * B + b] != v0[(size_t) 3 * B + b] || ll[b] != 0.0)) bad++;
            if (mask[b] && !(cov[d] < c0[d] && cov[d] > 0.0 && std::isfinite(ll[b]) && ll[b] != 0.0)) bad++;
          }
        }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
