// rbis_update_wide.hpp -- the indexed (+ orientation) update for index lists of seven to nine rows: RBISIndexedMeasurement /
// RBISIndexedPlusOrientationMeasurement::updateFilter (rbis.cpp:160-217) for the GPF's all_states list, velocity + chi + position
// (rgbd_gpf_lib.cpp:86-91), and whatever else pronto::indexed_measurement_t carries up to nine rows.  Launched from pb_update_wide.hip only.
//
// One lane per filter, as k_step_yawlock (pb_yawlock.hip): the measured columns W = P[:, idx], the m x m block P[idx, idx] and x[idx]
// are read with 8-byte loads in front of the one pass over the tile's 16-byte rows (they hit the cache the row pass fills); every
// gather of a lane is issued before its first store, so the update works in place.  Nine columns beside the state do not fit a lane's
// registers (the one-lane kernel spills at m = 5): W lives in LDS as [entry][lane], 135 doubles per lane for 15 states and 189 for 21
// (67.5 / 94.5 KiB per 64-lane workgroup at m = 9).  No lane reads another lane's entries, so there is no barrier.
//
// The index list is a kernel argument, the same for every lane.  The host turns it through the slot map Slots<NS>::T into a table of
// byte offsets (WideTab): every gather is a buffer load with a scalar offset, and in the row pass the (i, j) of every slot is a
// compile-time value.  No array is indexed at run time.
//
// wide_update_lane, the arithmetic of one lane, is measurement_update_cols' (rbis_device.hpp) term for term and compiles for the CPU
// too (tests/cpp/wide_update_host.cpp): it takes the gathered values, a W store and two functors that load and store a row.
#pragma once

#include "rbis_device.hpp"

namespace pb {

constexpr int WIDE_MIN_ROWS = 7, WIDE_MAX_ROWS = 9;
constexpr int WIDE_CHUNK = 16;  // rows in flight per lane while the tile streams through (64 VGPRs)

// Byte offsets into a tile of lane 0's copy of a component (row * 1024 + half * 8; a lane adds lane * 16), for the index list idx.
template <int NS, int M>
struct WideTab {
  unsigned col[NS][M];             // P(i, idx_k)
  unsigned blk[M * (M + 1) / 2];   // P(idx_k, idx_j), packed lower
  unsigned xm[M];                  // x[idx_k]
  int idx[M];
};
template <int NS>
PB_HD constexpr unsigned wide_offset(int comp)
{
  const int sl = Slots<NS>::T.slot_of[comp];
  return (unsigned) (sl >> 1) * 1024u + (unsigned) (sl & 1) * 8u;
}
template <int NS, int M>
inline WideTab<NS, M> make_wide_tab(const int *idx)
{
  using L = Lay<NS>;
  WideTab<NS, M> t;
  for (int k = 0; k < M; k++) {
    t.idx[k] = idx[k];
    t.xm[k] = wide_offset<NS>(L::OFF_VEC + idx[k]);
    for (int i = 0; i < NS; i++) t.col[i][k] = wide_offset<NS>(L::OFF_P + pk(i, idx[k]));
    for (int j = 0; j <= k; j++) t.blk[pk(k, j)] = wide_offset<NS>(L::OFF_P + pk(idx[k], idx[j]));
  }
  return t;
}

// W in a lane's own registers / in plain memory (the CPU tier)
template <int NS, int M>
struct WideRegs {
  double w[NS][M];
  PB_HD double get(int i, int k) const { return w[i][k]; }
  PB_HD void set(int i, int k, double v) { w[i][k] = v; }
  PB_HD void fence() const {}
};

// One lane's update.  In: q the prior quaternion; xm = x[idx]; z the measurement (entries at chi indices are ignored under ORIENT,
// rbis.cpp:206-208); qm the measured quaternion (ORIENT); S = R + P[idx, idx], packed lower; W = P[:, idx].  ldx(x, ll) fetches the
// prior state vector and log-likelihood when they are needed, behind the factorisation (held from the start they cost 44 registers
// through it, which spills for 21 states); ldrow(r) -> the pair (slot 2r, slot 2r + 1) of the prior, strow(r, a, b) stores the
// posterior's.  ldx comes before the first strow; ldrow and strow alternate in chunks of WIDE_CHUNK rows, each row loaded before
// it is stored.
template <int NS, int M, bool ORIENT, class WS, class LDX, class LDROW, class STROW>
PB_HD void wide_update_lane(const int (&idx)[M], double (&q)[4], const double (&xm)[M], const double (&z)[M], const double (&qm)[4],
                            double (&S)[M * (M + 1) / 2], WS &W, LDX ldx, LDROW ldrow, STROW strow, const Consts &k)
{
  using L = Lay<NS>;
  using SL = Slots<NS>;
  double dq[3] = { 0.0, 0.0, 0.0 };
  if constexpr (ORIENT) subtract_quats(qm, q, dq);  // rbis.cpp:199-205
  double resid[M];
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    double r = z[kk] - xm[kk];  // rbis.cpp:170
    if constexpr (ORIENT) {     // rbis.cpp:206-208 (the index is the same for every lane: a select, not an indexed read)
      const int c = idx[kk];
      r = (c == 6) ? dq[0] : (c == 7) ? dq[1] : (c == 8) ? dq[2] : r;
    }
    resid[kk] = r;
  }
  double d[M];
  ldlt<M>(S, d);
  // y = L^-1 r ; ll += -log det S - r^T S^-1 r with ONE log of the product of the pivots (rbis.cpp:142)
  double y[M], id[M], quad = 0.0, det = 1.0;
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    double s = resid[kk];
#pragma unroll
    for (int j = 0; j < kk; j++) s -= S[pk(kk, j)] * y[j];
    y[kk] = s;
    id[kk] = 1.0 / d[kk];
    det *= d[kk];
    quad += s * s * id[kk];
  }
  const double dll = -log(det) - quad;
  // W = P[:, idx] L^-T (row i: W_ik = P(i, idx_k) - sum_{j<k} W_ij L_kj) and dx = W D^-1 y
  double yd[M], dx[NS];
#pragma unroll
  for (int kk = 0; kk < M; kk++) yd[kk] = y[kk] * id[kk];
#pragma unroll
  for (int i = 0; i < NS; i++) {
    double w[M], s = 0.0;
    W.fence();  // (one row of W in registers at a time: the reads of later rows stay behind the writes of this one)
#pragma unroll
    for (int kk = 0; kk < M; kk++) w[kk] = W.get(i, kk);
#pragma unroll
    for (int kk = 0; kk < M; kk++) {
      double t = w[kk];
#pragma unroll
      for (int j = 0; j < kk; j++) t -= w[j] * S[pk(kk, j)];
      w[kk] = t;
      W.set(i, kk, t);
      s = (kk == 0) ? t * yd[0] : fma(t, yd[kk], s);
    }
    dx[i] = s;
  }
  double x[NS], ll;
  ldx(x, ll);
  ll += dll;
  add_delta<NS>(x, q, dx, k.chi_tol);
  // the posterior value of a slot from its prior value: P_ij = fma(-(W_ik / d_k), W_jk, P_ij) in increasing k
  auto post = [&](auto SLOT, double prior) {
    constexpr int comp = SL::T.comp_of[decltype(SLOT)::value];
    if constexpr (comp < 0) return 0.0;  // padding
    else if constexpr (comp >= L::OFF_P) {
      constexpr int i = pk_row(comp - L::OFF_P), j = pk_col(comp - L::OFF_P);
      double acc = prior;
#pragma unroll
      for (int kk = 0; kk < M; kk++) acc = fma(-(W.get(i, kk) * id[kk]), W.get(j, kk), acc);
      return acc;
    } else if constexpr (comp == L::OFF_LL) return ll;
    else if constexpr (comp >= L::OFF_QUAT) return q[comp - L::OFF_QUAT];
    else return x[comp - L::OFF_VEC];
  };
  constexpr int NCH = (SL::NROW + WIDE_CHUNK - 1) / WIDE_CHUNK;
  static_for<NCH>([&](auto CH) {
    constexpr int r0 = decltype(CH)::value * WIDE_CHUNK, r1 = (r0 + WIDE_CHUNK < SL::NROW) ? r0 + WIDE_CHUNK : SL::NROW;
    // (W is read again for every chunk: left to share the reads of earlier chunks, the compiler keeps most of W in registers)
    W.fence();
    decltype(ldrow(0)) buf[WIDE_CHUNK];
    static_for<r1 - r0>([&](auto R) { buf[decltype(R)::value] = ldrow(r0 + decltype(R)::value); });
    static_for<r1 - r0>([&](auto R) {
      constexpr int r = r0 + decltype(R)::value;
      const double a = post(std::integral_constant<int, 2 * r>{}, buf[decltype(R)::value].x);
      const double b = post(std::integral_constant<int, 2 * r + 1>{}, buf[decltype(R)::value].y);
      strow(r, a, b);
    });
  });
}

}  // namespace pb

#if defined(__HIPCC__)
#include "rbis_tile_io.hpp"

namespace pb {

constexpr int WIDE_GATHER_ROWS = 3;

// W in LDS, [entry][lane]: a lane reads and writes its own column only
template <int NS, int M>
struct WideLds {
  double (*w)[64];
  unsigned lane;
  __device__ __forceinline__ double get(int i, int k) const { return w[i * M + k][lane]; }
  __device__ __forceinline__ void set(int i, int k, double v) { w[i * M + k][lane] = v; }
  // reads behind it are issued again, writes in front of it are made: the pointer is an input, otherwise the compiler sees that the
  // asm cannot reach a __shared__ array whose address never leaves the kernel, and forwards all of W through registers
  __device__ __forceinline__ void fence() const { asm volatile("" ::"s"(w) : "memory"); }
};

// R: [M][B] (PB_R_DIAG), [M*M][B] column-major (PB_R_FULL) or rb (PB_R_DIAG_BROADCAST); mask [B] or NULL (0: the filter keeps its
// state bit for bit; where the posterior goes to another array than the prior's its rows are copied over, as yaw_copy does).
template <int NS, int M, bool ORIENT, int MH>
__global__ __launch_bounds__(64) void k_update_wide(const double *st, double *sto, int B, WideTab<NS, M> tab, const double *__restrict__ z,
                                                    const double *__restrict__ R, int rkind, DiagArg<M> rb, const double *__restrict__ qmeas,
                                                    const uint8_t *__restrict__ mask, Consts k)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  constexpr int LA = MemHint<MH>::LA, SA = MemHint<MH>::SA;
  __shared__ double wl[NS * M][64];
  const unsigned tile = xcd_workgroup(k), lane = threadIdx.x;
  const unsigned b = tile * 64u + lane;
  if (b >= (unsigned) B) return;
  const rsrc_t rs = mkbuf(reinterpret_cast<const char *>(st) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const rsrc_t ro = mkbuf(reinterpret_cast<char *>(sto) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const unsigned vo = lane * 16u;
  if (mask != nullptr && mask[b] == 0) {
    if (st != sto)
      for (int r = 0; r < S::NROW; r++) stg2<SA>(ro, (unsigned) r * 1024u, vo, ldg2<LA>(rs, (unsigned) r * 1024u, vo));
    return;
  }
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  // the measurement first (the only loads that are never cache-resident)
  const rsrc_t rz = mkbuf(z, (unsigned) M * B8);
  const rsrc_t rR = mkbuf(R, rkind == PB_R_DIAG ? (unsigned) M * B8 : (rkind == PB_R_FULL ? (unsigned) (M * M) * B8 : 0u));
  const rsrc_t rq = mkbuf(qmeas, ORIENT ? 4u * B8 : 0u);
  double zz[M], Sm[M * (M + 1) / 2], qm[4] = { 1.0, 0.0, 0.0, 0.0 };
#pragma unroll
  for (int i = 0; i < M; i++) {
    zz[i] = ldg(rz, i * B8, bo);
#pragma unroll
    for (int j = 0; j <= i; j++) {
      if (rkind == PB_R_DIAG_BROADCAST) Sm[pk(i, j)] = (i == j) ? rb.v[i] : 0.0;
      else if (rkind == PB_R_DIAG) Sm[pk(i, j)] = (i == j) ? ldg(rR, i * B8, bo) : 0.0;
      else Sm[pk(i, j)] = ldg(rR, (j * M + i) * B8, bo);
    }
  }
  if constexpr (ORIENT) {
#pragma unroll
    for (int i = 0; i < 4; i++) qm[i] = ldg(rq, i * B8, bo);
  }
  // the gathers: every 8-byte load of this lane's elements is issued before the first store of the row pass
  auto ld1 = [&](int comp) { return ldg<LA>(rs, wide_offset<NS>(comp), vo); };
  double q[4], xm[M];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = ld1(L::OFF_QUAT + i);
  WideLds<NS, M> W = { wl, lane };
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    xm[kk] = ldg<LA>(rs, tab.xm[kk], vo);
#pragma unroll
    for (int j = 0; j <= kk; j++) Sm[pk(kk, j)] += ldg<LA>(rs, tab.blk[pk(kk, j)], vo);  // rbis.cpp:134-135
  }
  // W, WIDE_GATHER_ROWS rows at a time, the loads of the next group in flight while this one goes to LDS (left alone, the scheduler
  // holds all NS * M loads in registers until the first LDS write: 378 VGPRs for 21 states, which spills)
  constexpr int G = WIDE_GATHER_ROWS, NG = (NS + G - 1) / G;
  double g[2][G][M];
  auto issue = [&](auto GI) {
    constexpr int gi = decltype(GI)::value;
#pragma unroll
    for (int r = 0; r < G; r++)
#pragma unroll
      for (int kk = 0; kk < M; kk++)
        if (gi * G + r < NS) g[gi & 1][r][kk] = ldg<LA>(rs, tab.col[gi * G + r][kk], vo);
  };
  issue(std::integral_constant<int, 0>{});
  static_for<NG>([&](auto GI) {
    constexpr int gi = decltype(GI)::value;
    W.fence();
    if constexpr (gi + 1 < NG) issue(std::integral_constant<int, gi + 1>{});
#pragma unroll
    for (int r = 0; r < G; r++)
#pragma unroll
      for (int kk = 0; kk < M; kk++)
        if (gi * G + r < NS) W.set(gi * G + r, kk, g[gi & 1][r][kk]);
  });
  wide_update_lane<NS, M, ORIENT>(
      tab.idx, q, xm, zz, qm, Sm, W,
      [&](double (&x)[NS], double &ll) {
#pragma unroll
        for (int i = 0; i < NS; i++) x[i] = ld1(L::OFF_VEC + i);
        ll = ld1(L::OFF_LL);
      },
      [&](int r) { return ldg2<LA>(rs, (unsigned) r * 1024u, vo); },
      [&](int r, double a, double c) { stg2<SA>(ro, (unsigned) r * 1024u, vo, d2_t{ a, c }); }, k);
}

}  // namespace pb
#endif
