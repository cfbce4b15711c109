// rbis_flow.hpp -- the optical-flow sigma-point update of one filter: RBISOpticalFlowMeasurement::measure and ::updateFilter
// (rbis_update_interface.cpp:111-138,160-260), the reference's only nonlinear measurement z = h(x), four rows.  Host/device like
// rbis_gpf.hpp: the kernel of rbis_flow_kernels.hpp runs flow_update_lane with its factor in LDS, g++ compiles the same text for
// tests/cpp/flow_host.cpp.
//
// The reference draws 2 n + 1 = 43 sigma points x +- sqrt(n + lambda) L e_i from the full Cholesky factor L of the 21 x 21 prior
// (:208-223).  h reads nothing below row 11 (omega, v, chi, Delta z) and L is lower triangular, so the points of columns 12 ... 20
// all measure z_0.  What remains is FLOW_COLS = 12 columns of the factor, an NS x 12 trapezoid L12 that depends on P[:, 0:12] only,
// and 25 evaluations of h.  With u+-_i = z+-_i - z_0, sd = sum_i (u+_i + u-_i), A = sum_i (u+_i u+_i^T + u-_i u-_i^T) and
// e = zhat - z_0 (the sums over i < 12; 42 = 2 n, whatever the context's size: a 15-state context is the reference's filter with
// zero bias blocks):
//   zhat = z_0 + e,   e = (Ws0 + 42 Wi - 1) z_0 + Wi sd                                                                  (:226-235)
//   Pzz  = R + Wi A - Wi (e sd^T + sd e^T) + (Wc0 + 42 Wi) e e^T                                                          (:241-249)
//   Pxz  = L12 D,  D_i = Wi sqrt(n + lambda) (z+_i - z-_i)                                                                (:250)
//   W = Pxz Lz^-T with Pzz = Lz Dz Lz^T (the unpivoted LDL^T of the other updates):  K = W Dz^-1 Lz^-1                    (:254)
//   x += W Dz^-1 Lz^-1 (z_meas - zhat),  P -= W Dz^-1 W^T                                                                 (:257-258)
// which is the reference's sum regrouped: nothing is approximated.  The regrouping is also where the accuracy comes from: the
// reference's weights are Ws0 ~ -1e6 and Wi ~ 2.4e4, and its own order cancels six digits in zhat and in the e e^T terms of Pzz;
// here Ws0 + 42 Wi (~ 1) and Wc0 + 42 Wi (~ 4) are formed with ONE rounding each (an fma of exact operands) and the sums run over
// differences from z_0.  The rank of the covariance downdate is that of Pzz, four, not twelve.
//
// The weights (lambda, Ws0, Wc0, Wi, sqrt(n + lambda)) are DATA: flow_weights() evaluates the reference's expressions (:199-206,221)
// once on the host, in double, in its order, and every consumer -- the kernel, the tests' witnesses -- takes those five doubles.
// fl(21e-6 - 21) + 21 is 2.1e-5 only to 1.7e-10, and that rounding has to be the same everywhere.
//
// As in the reference: posterior = prior, then vec += K innov with NO chi fold (:257; the next addState folds it), the quaternion and
// the log-likelihood keep the prior's bits (:163,190).  Unlike the reference: a pivot of the factor that is not positive (or not
// finite) in columns 0 ... 11 skips the update and reports the column; the reference goes on with whatever Eigen's failed LLT left
// in matrixL() unless that holds a NaN (:211-217).
#pragma once

#include "rbis_device.hpp"

namespace pb {

constexpr int FLOW_M = 4;        // rows of the measurement: ux, uy, theta, scale
constexpr int FLOW_COLS = 12;    // state rows h reads from lie in 0 ... 11
constexpr int FLOW_N_REF = 21;   // the reference's n (:197): its filter has 21 states
constexpr int FLOW_HEAD_QUAT = 1;  // flags bit 0 (PB_FLOW_HEAD_QUAT)

struct FlowCam {
  double r[3];                        // camera position in the body frame
  double zeta1[3], zeta2[3], eta[3];  // the reference's constructor arguments (rbis_update_interface.hpp:146-148)
};
struct FlowWeights {
  double lambda, Ws0, Wc0, Wi, sqrt_nl;
};
struct FlowMsg {
  double alpha1, alpha2, gamma;
};

// rbis_update_interface.cpp:199-206,221 with n = 21, in its order (the product is kept from being fused into the subtraction)
inline FlowWeights flow_weights()
{
  const int n = FLOW_N_REF;
  const double a2 = 1e-6, b = 2, k = 0;
  volatile double prod = a2 * (n + k);
  FlowWeights w;
  w.lambda = prod - n;
  volatile double npl = n + w.lambda;
  w.Ws0 = w.lambda / npl;
  volatile double one_a2 = 1 - a2;
  volatile double one_a2_b = one_a2 + b;
  w.Wc0 = w.lambda / npl + one_a2_b;
  volatile double two = 2 * npl;
  w.Wi = 1 / two;
  w.sqrt_nl = std::sqrt(npl);
  return w;
}

// entry of L12(i, k), k < FLOW_COLS, i >= k: the columns one behind the other, each from its diagonal down
template <int NS>
PB_HD constexpr int flow_e(int i, int k) { return k * NS - k * (k - 1) / 2 + (i - k); }
template <int NS>
struct FlowLen {
  static constexpr int value = FLOW_COLS * NS - FLOW_COLS * (FLOW_COLS - 1) / 2;  // 114 for 15 states, 186 for 21
};

// L12 in plain memory (the CPU tier)
template <int NS>
struct FlowMem {
  double v[FlowLen<NS>::value];
  PB_HD double get(int e) const { return v[e]; }
  PB_HD void set(int e, double x) { v[e] = x; }
  PB_HD void fence() const {}
};

// h of rbis_update_interface.cpp:111-138 as a functor over rows 0 ... 11 of a sigma point; at<I>: the point of column I of the factor
// (rows below I equal the head's), I = -1 the head itself, which comes first.
//   orientation (:113,117): RBIS(state_vec) is the identity quaternion folded with the point's chi, so R^T = Exp(chi)
//   when |chi| exceeds the fold tolerance and I otherwise; the head's quaternion enters under FLOW_HEAD_QUAT only.
//   Every P of :125-129 is a sum of outer products a b^T, so UnitZ . (R P R^T v) is a sum of (row 2 of R . a)(b . R^T v): the terms
//   below are the reference's, one for one, with the 3 x 3 products left unformed.
// Columns 9 ... 11 move Delta z only (x and y are not read): their points reuse the head's numerators.
struct FlowMeasure {
  FlowCam cam;
  FlowMsg msg;
  double tol;
  double qh[4];
  bool head_quat;
  double num0[4], add0[4], rr20;  // the head's: z_c = num_c / (Delta z + rr2) + add_c

  PB_HD void full(const double (&x)[FLOW_COLS], double (&num)[4], double (&add)[4], double &rr2) const
  {
    double q[4] = { 1.0, 0.0, 0.0, 0.0 };
    if (head_quat) { q[0] = qh[0]; q[1] = qh[1]; q[2] = qh[2]; q[3] = qh[3]; }
    double chi[3] = { x[6], x[7], x[8] };
    fold_chi(chi, q, tol);
    double Rw[9];  // body -> world; the reference's R (:117) is its transpose
    quat_to_rot(q, Rw);
    const double w[3] = { -x[0], -x[1], -x[2] };  // :118
    double Rr[3], v[3], tv[3], ww[3];
#pragma unroll
    for (int i = 0; i < 3; i++) Rr[i] = Rw[i] * cam.r[0] + Rw[3 + i] * cam.r[1] + Rw[6 + i] * cam.r[2];  // R * r
    v[0] = x[3] + (w[1] * Rr[2] - w[2] * Rr[1]);  // :119
    v[1] = x[4] + (w[2] * Rr[0] - w[0] * Rr[2]);
    v[2] = x[5] + (w[0] * Rr[1] - w[1] * Rr[0]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      tv[i] = Rw[3 * i] * v[0] + Rw[3 * i + 1] * v[1] + Rw[3 * i + 2] * v[2];  // R^T v
      ww[i] = Rw[3 * i] * w[0] + Rw[3 * i + 1] * w[1] + Rw[3 * i + 2] * w[2];  // w . (R a) = (R^T w) . a
    }
    const double c[3] = { Rw[2], Rw[5], Rw[8] };  // row 2 of R
    auto dot = [](const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double ce = dot(c, cam.eta), c1 = dot(c, cam.zeta1), c2 = dot(c, cam.zeta2);
    const double te = dot(cam.eta, tv), t1 = dot(cam.zeta1, tv), t2 = dot(cam.zeta2, tv);
    const double a1 = msg.alpha1, a2 = msg.alpha2, g = msg.gamma;
    rr2 = Rr[2];                                                                    // :123
    num[0] = ce * t2 + a2 * (c2 * te);                                              // P1, :125
    num[1] = ce * t1 + a1 * (c1 * te);                                              // P2, :126
    num[2] = .5 * (g + 1.) * (c2 * t1) + 5 * (g - 1.) * (c1 * t2);                  // Pt, :127 (5, not .5: the reference's text)
    num[3] = -(ce * te + .5 * (c1 * t1 + c2 * t2) + .5 * g * (c1 * t1 - c2 * t2));  // Ps, :128-129, with the sign of :134
    add[0] = -(a2 - 1) * dot(ww, cam.zeta2);                                        // :131
    add[1] = (a1 - 1) * dot(ww, cam.zeta1);                                         // :132
    add[2] = -dot(ww, cam.eta);                                                     // :133
    add[3] = 0.0;
  }
  template <int I>
  PB_HD void at(const double (&x)[FLOW_COLS], double (&z)[FLOW_M])
  {
    if constexpr (I >= 9) {
      const double lam = x[11] + rr20;
#pragma unroll
      for (int c = 0; c < 4; c++) z[c] = num0[c] / lam + add0[c];
    } else {
      double num[4], add[4], rr2;
      full(x, num, add, rr2);
      const double lam = x[11] + rr2;  // :121-123; no guard, as in the reference (:191-192)
#pragma unroll
      for (int c = 0; c < 4; c++) z[c] = num[c] / lam + add[c];
      if constexpr (I < 0) {
        rr20 = rr2;
#pragma unroll
        for (int c = 0; c < 4; c++) { num0[c] = num[c]; add0[c] = add[c]; }
      }
    }
  }
};

// One lane's update.  In: Lf holds P(i, k) at flow_e(i, k) and is left holding L12; x12 = rows 0 ... 11 of the prior vector; zm the
// measurement; Pzz = the measurement covariance R, packed lower; wt the five weights; meas the measurement functor (at<I>, above).
// Out: zhat (:236).  ldrow(r) -> the pair (slot 2r, slot 2r + 1) of the prior, strow(r, a, b) stores the posterior's; they alternate in
// chunks of FLOW_CHUNK rows, each row loaded before it is stored, and the first strow comes behind the last read of Lf.
// Returns 0, or 2 + k where pivot k is not positive or not finite: nothing was stored then (zhat is not written either).
constexpr int FLOW_CHUNK = 16;

template <int NS, class LS, class MEAS, class LDROW, class STROW>
PB_HD int flow_update_lane(LS &Lf, const double (&x12)[FLOW_COLS], const double (&zm)[FLOW_M], double (&Pzz)[FLOW_M * (FLOW_M + 1) / 2],
                           const FlowWeights &wt, MEAS &meas, double (&zhat)[FLOW_M], LDROW ldrow, STROW strow)
{
  using L = Lay<NS>;
  using SL = Slots<NS>;
  constexpr int M = FLOW_M, NC = FLOW_COLS;
  // ---- twelve columns of the Cholesky factor, left-looking and in place (:211) ----
  int status = 0;
  static_for<NC>([&](auto K) {
    constexpr int k = decltype(K)::value;
    if (status != 0) return;
    Lf.fence();
    double lk[k > 0 ? k : 1];
#pragma unroll
    for (int j = 0; j < k; j++) lk[j] = Lf.get(flow_e<NS>(k, j));
    double d = Lf.get(flow_e<NS>(k, k));
#pragma unroll
    for (int j = 0; j < k; j++) d = fma(-lk[j], lk[j], d);
    if (!(d > 0.0) || d > 1.7976931348623157e308) {
      status = 2 + k;
      return;
    }
    const double r = sqrt(d), ir = 1.0 / r;
    Lf.set(flow_e<NS>(k, k), r);
#pragma unroll
    for (int i = k + 1; i < NS; i++) {
      double s = Lf.get(flow_e<NS>(i, k));
#pragma unroll
      for (int j = 0; j < k; j++) s = fma(-Lf.get(flow_e<NS>(i, j)), lk[j], s);
      Lf.set(flow_e<NS>(i, k), s * ir);
    }
  });
  if (status != 0) return status;
  // ---- the sigma points of columns 0 ... 11 (:219-235) ----
  double z0[M];
  meas.template at<-1>(x12, z0);
  const double sc = wt.sqrt_nl, wd = wt.Wi * wt.sqrt_nl;
  double sd[M] = { 0.0, 0.0, 0.0, 0.0 }, A[M * (M + 1) / 2], D[NC][M];
#pragma unroll
  for (int p = 0; p < M * (M + 1) / 2; p++) A[p] = 0.0;
  static_for<NC>([&](auto I) {
    constexpr int i = decltype(I)::value;
    Lf.fence();
    double xp[NC], xn[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
      if (j < i) xp[j] = xn[j] = x12[j];
      else {
        const double l = Lf.get(flow_e<NS>(j, i));
        xp[j] = x12[j] + sc * l;  // :221
        xn[j] = x12[j] - sc * l;  // :222
      }
    }
    double zp[M], zn[M], up[M], un[M];
    meas.template at<i>(xp, zp);
    meas.template at<i>(xn, zn);
#pragma unroll
    for (int c = 0; c < M; c++) {
      up[c] = zp[c] - z0[c];
      un[c] = zn[c] - z0[c];
      sd[c] += up[c] + un[c];
      D[i][c] = wd * (zp[c] - zn[c]);
#pragma unroll
      for (int a = 0; a <= c; a++) A[pk(c, a)] += up[c] * up[a] + un[c] * un[a];
    }
  });
  // ---- zhat, Pzz and its factor (:226-249,254) ----
  constexpr double ALL = 2.0 * FLOW_N_REF;
  const double ws = fma(ALL, wt.Wi, wt.Ws0) - 1.0, wc = fma(ALL, wt.Wi, wt.Wc0);
  double e[M], innov[M];
#pragma unroll
  for (int c = 0; c < M; c++) {
    e[c] = fma(wt.Wi, sd[c], ws * z0[c]);
    zhat[c] = z0[c] + e[c];
    innov[c] = zm[c] - zhat[c];  // :257
  }
#pragma unroll
  for (int c = 0; c < M; c++)
#pragma unroll
    for (int a = 0; a <= c; a++) Pzz[pk(c, a)] += wt.Wi * (A[pk(c, a)] - (e[c] * sd[a] + sd[c] * e[a])) + wc * (e[c] * e[a]);
  double d[M], id[M], y[M], yd[M];
  ldlt<M>(Pzz, d);
#pragma unroll
  for (int c = 0; c < M; c++) {
    double s = innov[c];
#pragma unroll
    for (int j = 0; j < c; j++) s -= Pzz[pk(c, j)] * y[j];
    y[c] = s;
    id[c] = 1.0 / d[c];
    yd[c] = s * id[c];
  }
  // ---- W = L12 D Lz^-T, row by row, and dx = W Dz^-1 y ----
  double W[NS][M], dx[NS];
  Lf.fence();
#pragma unroll
  for (int a = 0; a < NS; a++) {
    double w[M] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int i = 0; i < (a < NC ? a + 1 : NC); i++) {
      const double l = Lf.get(flow_e<NS>(a, i));
#pragma unroll
      for (int c = 0; c < M; c++) w[c] = fma(l, D[i][c], w[c]);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < M; c++) {
      double t = w[c];
#pragma unroll
      for (int j = 0; j < c; j++) t -= w[j] * Pzz[pk(c, j)];
      w[c] = t;
      W[a][c] = t;
      s = fma(t, yd[c], s);
    }
    dx[a] = s;
  }
  Lf.fence();
  // ---- the posterior value of a slot from its prior value (:257-258): no fold, quaternion and log-likelihood pass through ----
  auto post = [&](auto SLOT, double prior) {
    constexpr int comp = SL::T.comp_of[decltype(SLOT)::value];
    if constexpr (comp < 0) return 0.0;  // padding
    else if constexpr (comp >= L::OFF_P) {
      constexpr int i = pk_row(comp - L::OFF_P), j = pk_col(comp - L::OFF_P);
      double acc = prior;
#pragma unroll
      for (int c = 0; c < M; c++) acc = fma(-(W[i][c] * id[c]), W[j][c], acc);
      return acc;
    } else if constexpr (comp >= L::OFF_QUAT) return prior;
    else return prior + dx[comp - L::OFF_VEC];
  };
  constexpr int NCH = (SL::NROW + FLOW_CHUNK - 1) / FLOW_CHUNK;
  static_for<NCH>([&](auto CH) {
    constexpr int r0 = decltype(CH)::value * FLOW_CHUNK, r1 = (r0 + FLOW_CHUNK < SL::NROW) ? r0 + FLOW_CHUNK : SL::NROW;
    decltype(ldrow(0)) buf[FLOW_CHUNK];
    static_for<r1 - r0>([&](auto R) { buf[decltype(R)::value] = ldrow(r0 + decltype(R)::value); });
    static_for<r1 - r0>([&](auto R) {
      constexpr int r = r0 + decltype(R)::value;
      const double a = post(std::integral_constant<int, 2 * r>{}, buf[decltype(R)::value].x);
      const double b = post(std::integral_constant<int, 2 * r + 1>{}, buf[decltype(R)::value].y);
      strow(r, a, b);
    });
  });
  return 0;
}

}  // namespace pb
