// flow_host.cpp -- the per-lane function of the optical-flow update (pronto_amd/csrc/rbis_flow.hpp) compiled by g++: the same text
// k_update_flow runs, with the factor in plain memory and a filter's tile rows in a small array.  Built as a shared object for
// tests/test_flow_host.py, and with -DFLOW_HOST_MAIN as a stand-alone program that runs a fixed batch (for
// -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pronto_amd/csrc/rbis_flow.hpp"

using namespace pb;

struct Pair {
  double x, y;
};

// vec [NS][B], quat [4][B], ll [B], P [NS][NS][B] (the lower triangle is read), flow [7][B], R [16][B] column-major, cam = r, zeta1,
// zeta2, eta, wts = the five weights -> the posterior in the same layouts (P: both triangles), zhat [4][B], status [B]
template <int NS>
static void update_ns(int B, const double *vec, const double *quat, const double *ll, const double *P, const double *flow, const double *R,
                      const double *cam, const double *wts, double tol, int flags, double *vec_out, double *quat_out, double *ll_out,
                      double *P_out, double *zhat_out, int32_t *status)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  FlowWeights wt = { wts[0], wts[1], wts[2], wts[3], wts[4] };
  for (int b = 0; b < B; b++) {
    double comp[L::NC], slot[S::NSLOT];
    for (int i = 0; i < NS; i++) comp[L::OFF_VEC + i] = vec[(size_t) i * B + b];
    for (int i = 0; i < 4; i++) comp[L::OFF_QUAT + i] = quat[(size_t) i * B + b];
    comp[L::OFF_LL] = ll[b];
    for (int i = 0; i < NS; i++)
      for (int j = 0; j <= i; j++) comp[L::OFF_P + pk(i, j)] = P[((size_t) i * NS + j) * B + b];
    for (int s = 0; s < S::NSLOT; s++) slot[s] = S::T.comp_of[s] < 0 ? 0.0 : comp[S::T.comp_of[s]];
    FlowMem<NS> Lf;
    for (int k = 0; k < FLOW_COLS; k++)
      for (int i = k; i < NS; i++) Lf.set(flow_e<NS>(i, k), comp[L::OFF_P + pk(i, k)]);
    double x12[FLOW_COLS], zm[4], Pzz[10], zhat[4] = { NAN, NAN, NAN, NAN };
    for (int i = 0; i < FLOW_COLS; i++) x12[i] = comp[L::OFF_VEC + i];
    FlowMeasure meas;
    for (int i = 0; i < 3; i++) {
      meas.cam.r[i] = cam[i];
      meas.cam.zeta1[i] = cam[3 + i];
      meas.cam.zeta2[i] = cam[6 + i];
      meas.cam.eta[i] = cam[9 + i];
    }
    meas.msg = FlowMsg{ flow[(size_t) 4 * B + b], flow[(size_t) 5 * B + b], flow[(size_t) 6 * B + b] };
    meas.tol = tol;
    meas.head_quat = (flags & FLOW_HEAD_QUAT) != 0;
    for (int i = 0; i < 4; i++) {
      meas.qh[i] = comp[L::OFF_QUAT + i];
      zm[i] = flow[(size_t) i * B + b];
      for (int j = 0; j <= i; j++) Pzz[pk(i, j)] = R[((size_t) j * 4 + i) * B + b];
    }
    status[b] = flow_update_lane<NS>(
        Lf, x12, zm, Pzz, wt, meas, zhat, [&](int r) { return Pair{ slot[2 * r], slot[2 * r + 1] }; },
        [&](int r, double a, double c) {
          slot[2 * r] = a;
          slot[2 * r + 1] = c;
        });
    for (int s = 0; s < S::NSLOT; s++)
      if (S::T.comp_of[s] >= 0) comp[S::T.comp_of[s]] = slot[s];
    for (int i = 0; i < NS; i++) vec_out[(size_t) i * B + b] = comp[L::OFF_VEC + i];
    for (int i = 0; i < 4; i++) quat_out[(size_t) i * B + b] = comp[L::OFF_QUAT + i];
    ll_out[b] = comp[L::OFF_LL];
    for (int i = 0; i < NS; i++)
      for (int j = 0; j < NS; j++) P_out[((size_t) i * NS + j) * B + b] = comp[L::OFF_P + pk(i, j)];
    for (int i = 0; i < 4; i++) zhat_out[(size_t) i * B + b] = zhat[i];
  }
}

extern "C" {
void flow_host_weights(double out[5])
{
  const FlowWeights w = flow_weights();
  out[0] = w.lambda; out[1] = w.Ws0; out[2] = w.Wc0; out[3] = w.Wi; out[4] = w.sqrt_nl;
}
int flow_host_update(int ns, int B, const double *vec, const double *quat, const double *ll, const double *P, const double *flow, const double *R,
                     const double *cam, const double *wts, double tol, int flags, double *vec_out, double *quat_out, double *ll_out, double *P_out,
                     double *zhat_out, int32_t *status)
{
  if (ns == 15) update_ns<15>(B, vec, quat, ll, P, flow, R, cam, wts, tol, flags, vec_out, quat_out, ll_out, P_out, zhat_out, status);
  else if (ns == 21) update_ns<21>(B, vec, quat, ll, P, flow, R, cam, wts, tol, flags, vec_out, quat_out, ll_out, P_out, zhat_out, status);
  else return 1;
  return 0;
}
}

#ifdef FLOW_HOST_MAIN
// a fixed batch through both state sizes and both flags: diagonally dominant P, one filter with P = 0, one with a negative pivot 7
int main()
{
  const int B = 4;
  double wts[5];
  flow_host_weights(wts);
  const double c = std::cos(3.2415926535897931), s = std::sin(3.2415926535897931);
  const double cam[12] = { 0.1, 0.02, -0.05, 1, 0, 0, 0, c, -s, 0, s, c };
  for (int ns : { 15, 21 })
    for (int flags = 0; flags < 2; flags++) {
      std::vector<double> vec((size_t) ns * B, 0.1), quat(4 * B, 0.0), ll(B, -1.5), P((size_t) ns * ns * B, 0.0), flow(7 * B, 1.0), R(16 * B, 0.0),
          vo(vec.size()), qo(quat.size()), lo(B), Po(P.size()), zh(4 * B);
      std::vector<int32_t> status(B);
      for (int b = 0; b < B; b++) {
        quat[b] = 0.8; quat[(size_t) 3 * B + b] = 0.6;
        vec[(size_t) 11 * B + b] = 2.0 + b;
        for (int i = 6; i < 9; i++) vec[(size_t) i * B + b] = 1e-9;
        for (int i = 0; i < 4; i++) {
          flow[(size_t) i * B + b] = 0.05 * (i + 1);
          R[((size_t) i * 4 + i) * B + b] = 0.0025;
        }
        for (int i = 0; i < ns; i++)
          for (int j = 0; j < ns; j++) P[((size_t) i * ns + j) * B + b] = b == 2 ? 0.0 : (i == j ? 0.01 * (1 + i) : 0.0004);
      }
      P[((size_t) 7 * ns + 7) * B + 3] = -1.0;
      if (flow_host_update(ns, B, vec.data(), quat.data(), ll.data(), P.data(), flow.data(), R.data(), cam, wts, 1e-6, flags, vo.data(), qo.data(),
                           lo.data(), Po.data(), zh.data(), status.data()))
        return 2;
      if (status[0] != 0 || status[1] != 0 || status[2] != 2 || status[3] != 9) return 3;
      for (int i = 0; i < ns; i++)
        if (!(std::fabs(vo[(size_t) i * B]) < 1e300) || vo[(size_t) i * B + 2] != vec[(size_t) i * B + 2]) return 4;
      if (!(Po[0] > 0.0 && Po[0] < P[0])) return 5;
    }
  printf("ok\n");
  return 0;
}
#endif
