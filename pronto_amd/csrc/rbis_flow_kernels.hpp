// rbis_flow_kernels.hpp -- k_update_flow<NS, MH>: the optical-flow sigma-point update (rbis_flow.hpp; RBISOpticalFlowMeasurement,
// rbis_update_interface.cpp:109-260) of a batch, one launch per message.  Launched from pb_flow.hip only.
//
// One lane per filter, the mapping of k_update_wide (rbis_update_wide.hpp): the twelve measured columns P[:, 0:12]
// from the diagonal down, rows 0 ... 11 of x and the quaternion are read with 8-byte loads in front of the one pass over the tile's
// 16-byte rows; every gather of a lane is issued before its first store, so the update works in place.  The columns go to LDS as
// [entry][lane] and are factored there (114 doubles per lane for 15 states, 186 for 21: 57 / 93 KiB per 64-lane workgroup); a lane
// reads and writes its own column only, so there is no barrier.  What is left of the arithmetic -- the 25 evaluations of h, the
// 4 x 4 factor, W = L12 D Lz^-T (NS x 4) -- stays in registers, and the row pass is k_update_wide's with four columns.
// Every offset is a compile-time value: the layout is fixed, so there is no table and no policy entry.
#pragma once

#include "rbis_flow.hpp"
#include "rbis_tile_io.hpp"

namespace pb {

// byte offset into a tile of lane 0's copy of a component (a lane adds lane * 16)
template <int NS>
PB_HD constexpr unsigned flow_offset(int comp)
{
  const int sl = Slots<NS>::T.slot_of[comp];
  return (unsigned) (sl >> 1) * 1024u + (unsigned) (sl & 1) * 8u;
}

// L12 in LDS, [entry][lane]
struct FlowLds {
  double (*w)[64];
  unsigned lane;
  __device__ __forceinline__ double get(int e) const { return w[e][lane]; }
  __device__ __forceinline__ void set(int e, double v) { w[e][lane] = v; }
  // (reads behind it are issued again, writes in front of it are made: WideLds::fence, rbis_update_wide.hpp)
  __device__ __forceinline__ void fence() const { asm volatile("" ::"s"(w) : "memory"); }
};

// flow [7][B]: ux, uy, theta, scale, alpha1, alpha2, gamma; R: [4][B] (PB_R_DIAG), [16][B] column-major (PB_R_FULL) or rb
// (PB_R_DIAG_BROADCAST); mask [B] or NULL (0: the filter keeps its state bit for bit; where the posterior goes to another array than
// the prior's its rows are copied over); zhat_out [4][B] or NULL (written for status 0 only); status_out [B] or NULL.
template <int NS, int MH>
__global__ __launch_bounds__(64) void k_update_flow(const double *st, double *sto, int B, const double *__restrict__ flow,
                                                    const double *__restrict__ R, int rkind, DiagArg<FLOW_M> rb,
                                                    const uint8_t *__restrict__ mask, FlowCam cam, FlowWeights wt, int flags,
                                                    double *__restrict__ zhat_out, int32_t *__restrict__ status_out, Consts k)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  constexpr int LA = MemHint<MH>::LA, SA = MemHint<MH>::SA, M = FLOW_M;
  __shared__ double lf[FlowLen<NS>::value][64];
  const unsigned tile = xcd_workgroup(k), lane = threadIdx.x;
  const unsigned b = tile * 64u + lane;
  // (the padding lanes of the last tile are nobody's: every reader of a state array or a checkpoint slot stops at B, so they are not
  // copied to an output slot either, as in k_update_wide)
  if (b >= (unsigned) B) return;
  const rsrc_t rs = mkbuf(reinterpret_cast<const char *>(st) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const rsrc_t ro = mkbuf(reinterpret_cast<char *>(sto) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const unsigned vo = lane * 16u;
  auto keep = [&](int status) {  // posterior = prior
    if (status_out != nullptr) status_out[b] = status;
    if (st != sto)
      for (int r = 0; r < S::NROW; r++) stg2<SA>(ro, (unsigned) r * 1024u, vo, ldg2<LA>(rs, (unsigned) r * 1024u, vo));
  };
  if (mask != nullptr && mask[b] == 0) {
    keep(1);
    return;
  }
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  // the message first (the only loads that are never cache-resident)
  const rsrc_t rf = mkbuf(flow, 7u * B8);
  const rsrc_t rR = mkbuf(R, rkind == PB_R_DIAG ? (unsigned) M * B8 : (rkind == PB_R_FULL ? (unsigned) (M * M) * B8 : 0u));
  double zm[M], Pzz[M * (M + 1) / 2];
  FlowMeasure meas;
  meas.cam = cam;
  meas.tol = k.chi_tol;
  meas.head_quat = (flags & FLOW_HEAD_QUAT) != 0;
#pragma unroll
  for (int i = 0; i < M; i++) {
    zm[i] = ldg(rf, i * B8, bo);
#pragma unroll
    for (int j = 0; j <= i; j++) {
      if (rkind == PB_R_DIAG_BROADCAST) Pzz[pk(i, j)] = (i == j) ? rb.v[i] : 0.0;
      else if (rkind == PB_R_DIAG) Pzz[pk(i, j)] = (i == j) ? ldg(rR, i * B8, bo) : 0.0;
      else Pzz[pk(i, j)] = ldg(rR, (j * M + i) * B8, bo);
    }
  }
  meas.msg.alpha1 = ldg(rf, 4 * B8, bo);
  meas.msg.alpha2 = ldg(rf, 5 * B8, bo);
  meas.msg.gamma = ldg(rf, 6 * B8, bo);
  // the gathers: every 8-byte load of this lane's elements is issued before the first store of the row pass
  auto ld1 = [&](int comp) { return ldg<LA>(rs, flow_offset<NS>(comp), vo); };
  double x12[FLOW_COLS];
#pragma unroll
  for (int i = 0; i < 4; i++) meas.qh[i] = ld1(L::OFF_QUAT + i);
#pragma unroll
  for (int i = 0; i < FLOW_COLS; i++) x12[i] = ld1(L::OFF_VEC + i);
  // P[:, 0:12] a column at a time, the loads of the next column in flight while this one goes to LDS (left alone, the scheduler
  // holds every load in registers until the first LDS write)
  FlowLds Lf = { lf, lane };
  double g[2][NS];
  auto issue = [&](auto KI) {
    constexpr int kk = decltype(KI)::value;
#pragma unroll
    for (int i = kk; i < NS; i++) g[kk & 1][i] = ld1(L::OFF_P + pk(i, kk));
  };
  issue(std::integral_constant<int, 0>{});
  static_for<FLOW_COLS>([&](auto KI) {
    constexpr int kk = decltype(KI)::value;
    Lf.fence();
    if constexpr (kk + 1 < FLOW_COLS) issue(std::integral_constant<int, kk + 1>{});
#pragma unroll
    for (int i = kk; i < NS; i++) Lf.set(flow_e<NS>(i, kk), g[kk & 1][i]);
  });
  double zhat[M];
  const int status = flow_update_lane<NS>(
      Lf, x12, zm, Pzz, wt, meas, zhat, [&](int r) { return ldg2<LA>(rs, (unsigned) r * 1024u, vo); },
      [&](int r, double a, double c) { stg2<SA>(ro, (unsigned) r * 1024u, vo, d2_t{ a, c }); });
  if (status != 0) {
    keep(status);
    return;
  }
  if (status_out != nullptr) status_out[b] = 0;
  if (zhat_out != nullptr) {
#pragma unroll
    for (int i = 0; i < M; i++) zhat_out[(size_t) i * B + b] = zhat[i];
  }
}

}  // namespace pb
