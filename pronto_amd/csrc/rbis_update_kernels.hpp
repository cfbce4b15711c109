// rbis_update_kernels.hpp -- the stand-alone indexed update kernels: k_update_lane (compile-time index list, one lane per filter),
// k_update_lane_rt (run-time list, 15 states) and k_update_quad (21 states, four waves per tile, rbis_quad.hpp).  Launched from
// pb_update_ct.hip and pb_update.hip.  Tile I/O and argument structs: rbis_tile_io.hpp.
#pragma once

#include "rbis_tile_io.hpp"
#include "rbis_coop.hpp"
#include "rbis_quad.hpp"

namespace pb {

// (The generic run-time-index update of a 21-state batch is k_update_quad_rt, rbis_quad_rt.hpp; the 15-state one
//  k_update_lane_rt below (m <= 4) and k_update_coop_rt (m = 5, 6; rbis_quad_rt.hpp).  Round 1 / 2 gathered the measured columns with 8-byte run-time-slot loads and streamed the
//  covariance through one wave, k_update<NS, M, ORIENT>: 54-80 us for 21 states at 64k filters, retired in round 3.)

// Stand-alone indexed update, one lane per filter, COMPILE-TIME index list anywhere in the state (15 states: the whole
// filter lives in registers, as in k_step): one coalesced round trip of the state and the in-register update of the fused
// step (measurement_update) instead of the generic k_update's run-time column gather, which reads the measured columns a
// second time.  Diagonal (per filter or one for all) or full per-filter R, skip mask, broadcast z: CorrArgs.
template <int NS, int M, class IDXT, int MH = MH_DEFAULT>
__global__ __launch_bounds__(64, 1) void k_update_lane(const double *st, double *sto, int B, Consts k, CorrArgs ca)
{
  using L = Lay<NS>;
  constexpr Idx<M> idx = IDXT::value;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + threadIdx.x;
  if (b >= (unsigned) B) return;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA> io(st, sto, tile, threadIdx.x);
  const bool upd = (ca.mask2 == nullptr) || (ca.mask2[b] != 0);  // 0 = handler returned NULL for this filter
  // the measurement first (the only loads that are never cache-resident), then the state rows
  const rsrc_t rz = mkbuf(ca.z2, ca.zbc ? 0u : (unsigned) M * B8);
  const rsrc_t rr = mkbuf(ca.rfull ? ca.rfull : ca.r2, ca.rfull ? (unsigned) (M * M) * B8 : (ca.r2 ? (unsigned) M * B8 : 0u));
  double z[M], R[M * (M + 1) / 2];
#pragma unroll
  for (int i = 0; i < M; i++) {
    z[i] = ca.zbc ? ca.zb2[i] : ldg(rz, i * B8, bo);
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double r;
      if (ca.rfull) r = ldg(rr, (j * M + i) * B8, bo);
      else if (i != j) r = 0.0;
      else r = ca.r2 ? ldg(rr, i * B8, bo) : ca.rb2[i];
      R[pk(i, j)] = upd ? r : (i == j ? 1.0 : 0.0);  // benign R for skipped filters (their block may hold anything)
    }
  }
  io.template need<0, Slots<NS>::NROW>();
  double x[NS], q[4], ll, P[L::NP];
#pragma unroll
  for (int i = 0; i < NS; i++) x[i] = io.ld(L::OFF_VEC + i);
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = io.ld(L::OFF_QUAT + i);
  ll = io.ld(L::OFF_LL);
#pragma unroll
  for (int i = 0; i < L::NP; i++) P[i] = io.ld(L::OFF_P + i);
  double resid[M], S[M * (M + 1) / 2];
#pragma unroll
  for (int i = 0; i < M; i++) {
    resid[i] = upd ? z[i] - x[idx.v[i]] : 0.0;                                   // rbis.cpp:170
#pragma unroll
    for (int j = 0; j <= i; j++) S[pk(i, j)] = P[pk(idx.v[i], idx.v[j])] + R[pk(i, j)];  // rbis.cpp:134-135
  }
  measurement_update<NS, M>(x, q, P, ll, resid, S, IDXT{}, k, [&io](int pi, double v) { io.st(L::OFF_P + pi, v); }, upd);
#pragma unroll
  for (int i = 0; i < NS; i++) io.st(L::OFF_VEC + i, x[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) io.st(L::OFF_QUAT + i, q[i]);
  io.st(L::OFF_LL, ll);
}

// Column c (wave-uniform) of the packed covariance into column KK of W, with the residual and row KK of S = R + P[idx, idx]:
// a chain of scalar compares over the compile-time candidates CC, CC + 1, ... (one branch taken, NS register moves).
template <int NS, int M, int KK, int CC, bool ORIENT>
__device__ __forceinline__ void pick_column(int c, const double (&P)[NS * (NS + 1) / 2], const double (&x)[NS], const double (&zz)[M],
                                            const double (&dq)[3], bool upd, double (&W)[NS][M], double (&resid)[M],
                                            double (&S)[M * (M + 1) / 2])
{
  if constexpr (CC < NS) {
    if (c == CC) {
      // (a distinct marker per branch: otherwise the identical branch bodies are merged into ONE body that loads through a
      // selected address, which pins the whole covariance in scratch memory)
      asm volatile("; column %0 -> %1" ::"n"(CC), "n"(KK));
#pragma unroll
      for (int i = 0; i < NS; i++) W[i][KK] = P[pk(i, CC)];
      double r = zz[KK] - x[CC];                                    // rbis.cpp:170
      if constexpr (ORIENT && CC >= 6 && CC <= 8) r = dq[CC - 6];   // rbis.cpp:206-208
      resid[KK] = upd ? r : 0.0;
#pragma unroll
      for (int j = 0; j < KK; j++) S[pk(KK, j)] += W[CC][j];        // P[idx_KK, idx_j]: row CC of an earlier column
      S[pk(KK, KK)] += P[pk(CC, CC)];
      asm volatile("; column %0 -> %1 done" ::"n"(CC), "n"(KK));  // (common-tail sinking stops here)
    } else {
      pick_column<NS, M, KK, CC + 1, ORIENT>(c, P, x, zz, dq, upd, W, resid, S);
    }
  }
}

// The generic update for 15 states: RUN-TIME index list (any indices, m = 1..6, diagonal / broadcast / full R, orientation
// residual, skip mask -- RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement::updateFilter,
// rbis_update_interface.cpp:54-107) on the same one-lane in-register scheme.  The index list is a kernel argument, i.e.
// wave-uniform: each measured column is picked by a scalar branch over the 15 compile-time candidates (15 register moves
// taken, nothing gathered from memory), then measurement_update_cols runs as for a compile-time list -- so the result is
// bit-identical to k_update_lane's for the same list.  21 states do not fit one lane's registers: k_update stays for them.
template <int NS, int M, bool ORIENT, int MH = MH_DEFAULT>
__global__ __launch_bounds__(64, 1) void k_update_lane_rt(const double *st, double *sto, int B, IdxArg<M> idx,
                                                          const double *__restrict__ z, const double *__restrict__ R,
                                                          int rkind, DiagArg<M> rb, const double *__restrict__ qmeas,
                                                          const uint8_t *__restrict__ mask, Consts k)
{
  using L = Lay<NS>;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + threadIdx.x;
  if (b >= (unsigned) B) return;
  const bool upd = (mask == nullptr) || (mask[b] != 0);  // 0 = handler returned NULL for this filter
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA> io(st, sto, tile, threadIdx.x);
  const rsrc_t rz = mkbuf(z, (unsigned) M * B8);
  const rsrc_t rR = mkbuf(R, rkind == PB_R_DIAG ? (unsigned) M * B8 : (rkind == PB_R_FULL ? (unsigned) (M * M) * B8 : 0u));
  const rsrc_t rq = mkbuf(qmeas, ORIENT ? 4u * B8 : 0u);
  double zz[M], S[M * (M + 1) / 2], qm[4] = { 1.0, 0.0, 0.0, 0.0 };
#pragma unroll
  for (int i = 0; i < M; i++) {
    zz[i] = ldg(rz, i * B8, bo);
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double r;
      if (rkind == PB_R_DIAG_BROADCAST) r = (i == j) ? rb.v[i] : 0.0;
      else if (rkind == PB_R_DIAG) r = (i == j) ? ldg(rR, i * B8, bo) : 0.0;
      else r = ldg(rR, (j * M + i) * B8, bo);
      S[pk(i, j)] = upd ? r : (i == j ? 1.0 : 0.0);  // benign R for skipped filters (their R block may hold anything)
    }
  }
  if constexpr (ORIENT) {
#pragma unroll
    for (int i = 0; i < 4; i++) qm[i] = ldg(rq, i * B8, bo);
  }
  io.template need<0, Slots<NS>::NROW>();
  double x[NS], q[4], ll, P[L::NP];
#pragma unroll
  for (int i = 0; i < NS; i++) x[i] = io.ld(L::OFF_VEC + i);
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = io.ld(L::OFF_QUAT + i);
  ll = io.ld(L::OFF_LL);
#pragma unroll
  for (int i = 0; i < L::NP; i++) P[i] = io.ld(L::OFF_P + i);
  double dq[3] = { 0.0, 0.0, 0.0 };
  if constexpr (ORIENT) subtract_quats(qm, q, dq);  // rbis.cpp:199-205
  // the measured columns, the measured states and P[idx, idx], by scalar branches on the (uniform) indices
  double W[NS][M], resid[M];
  static_for<M>([&](auto KK) { pick_column<NS, M, decltype(KK)::value, 0, ORIENT>(idx.v[decltype(KK)::value], P, x, zz, dq, upd, W, resid, S); });
  measurement_update_cols<NS, M>(x, q, P, ll, resid, S, W, k, [&io](int pi, double v) { io.st(L::OFF_P + pi, v); }, upd);
#pragma unroll
  for (int i = 0; i < NS; i++) io.st(L::OFF_VEC + i, x[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) io.st(L::OFF_QUAT + i, q[i]);
  io.st(L::OFF_LL, ll);
}

// Stand-alone indexed (+ orientation) update of a 21-state batch on the four-wave mapping (rbis_quad.hpp, quad_upd_*): the
// handlers' index lists as compile-time c-state indices, diagonal R, one barrier, one state round trip at two waves per SIMD.
template <class CORR, int MH = MH_DEFAULT>
__global__ __launch_bounds__(256, 2) void k_update_quad(const double *st, double *sto, int B, Consts k, CorrArgs ca)
{
  using SL = Slots<21>;
  __shared__ double xch[QuadU<CORR>::NXCH][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<21, MemHint<MH>::LA, MemHint<MH>::SA> io(st, sto, tile, lane);
  // an update that no filter of this tile takes, in place: all four waves see the same mask bytes and leave together (k_step_coop)
  if (st == sto && ca.mask2 != nullptr && __ballot(b < (unsigned) B && ca.mask2[b < (unsigned) B ? b : 0u] != 0) == 0ull) return;
  auto inputs = [&](bool meas) {
    CorrInputs cin;
    const rsrc_t rz = mkbuf(ca.z2, (unsigned) CORR::M * B8);
    const rsrc_t rr = mkbuf(ca.r2, ca.r2 ? (unsigned) CORR::M * B8 : 0u);
    const rsrc_t rq2 = mkbuf(ca.qm2, CORR::ORIENT ? 4u * B8 : 0u);
#pragma unroll
    for (int i = 0; i < CORR::M; i++) {
      cin.z[i] = meas ? (ca.zbc ? ca.zb2[i] : ldg(rz, i * B8, bo)) : 0.0;
      cin.rd[i] = meas ? (ca.r2 ? ldg(rr, i * B8, bo) : ca.rb2[i]) : 1.0;
    }
    if (meas && ca.rfull != nullptr) {  // full R (wave-uniform branch): diagonal + strictly-lower part
      const rsrc_t rf = mkbuf(ca.rfull, (unsigned) (CORR::M * CORR::M) * B8);
#pragma unroll
      for (int i = 0; i < CORR::M; i++) {
        cin.rd[i] = ldg(rf, (unsigned) (i * CORR::M + i) * B8, bo);
#pragma unroll
        for (int j = 0; j < i; j++) cin.ro[i * (i - 1) / 2 + j] = ldg(rf, (unsigned) (j * CORR::M + i) * B8, bo);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) cin.qm[i] = (CORR::ORIENT && meas) ? (ca.zbc ? ca.qb2[i] : ldg(rq2, i * B8, bo)) : 0.0;
    cin.upd = (b < (unsigned) B) && (ca.mask2 == nullptr || ca.mask2[b] != 0);
    return cin;
  };
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  auto xwr = [lane](int s, double v) { xch[s][lane] = v; };
  if (role == 0) {  // (the measurement blocks are requested first, see k_step_quad)
    const CorrInputs cin = inputs(true);
    io.template need<SL::QROW[0], SL::QROW[1]>();
    quad_upd_cc<CORR>(ld, stf, xwr, xrd, sync, cin, k);
  } else if (role == 1) {
    const CorrInputs cin = inputs(false);
    io.template need<SL::QROW[1], SL::QROW[2]>();
    quad_upd_cb<CORR>(ld, stf, xwr, xrd, sync, cin, k);
  } else if (role == 2) {
    const CorrInputs cin = inputs(false);
    io.template need<SL::QROW[2], SL::QROW[3]>();
    quad_upd_passive<CORR, 0>(ld, stf, xwr, xrd, sync, cin, k);
  } else {
    const CorrInputs cin = inputs(false);
    io.template need<SL::QROW[3], SL::QROW[4]>();
    quad_upd_passive<CORR, 1>(ld, stf, xwr, xrd, sync, cin, k);
  }
}

}  // namespace pb
