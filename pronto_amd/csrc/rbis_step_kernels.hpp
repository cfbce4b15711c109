// rbis_step_kernels.hpp -- the step kernels: k_step (one lane per filter), k_step_coop (two waves per tile, rbis_coop.hpp) and
// k_step_quad (four waves per tile, rbis_quad.hpp), and the variants that also keep the predicted posterior (k_step_coop_pred,
// k_step_coop_corr_pred, k_step_quad_pred).  Launched from pb_step.hip, pb_step_pred.hip, pb_step_corr_pred.hip and pb_update_ct.hip
// (k_step_coop with PREDICT = false).  Tile I/O and argument structs: rbis_tile_io.hpp.
#pragma once

#include "rbis_tile_io.hpp"
#include "rbis_coop.hpp"
#include "rbis_quad.hpp"

namespace pb {

// RBISIMUProcessStep::updateFilter [+ RBISIndexedMeasurement::updateFilter with idx = {3,4,5}, diagonal R]
// (rbis_update_interface.cpp:30-52, :54-95).  The BASELINE hot step: 2*(n+4+1+n(n+1)/2)*8 + 56 + 48 bytes/filter.
// One lane per filter, one tile per 64-thread workgroup.
template <int NS, bool UPDATE, int MH = MH_DEFAULT>
__global__ __launch_bounds__(PB_STEP_BLOCK, 1) void k_step(const double *st, double *sto, int B,
                                                const double *__restrict__ imu, const double *__restrict__ lo,
                                                const uint8_t *__restrict__ mask, double qg, double qa, double qbg,
                                                double qba, Consts k, StepBcast bc)
{
  using L = Lay<NS>;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + threadIdx.x;
  if (b >= (unsigned) B) return;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA> io(st, sto, tile, threadIdx.x);  // posterior: in place or a checkpoint slot
  const rsrc_t ri = mkbuf(imu, 7u * B8);
  const rsrc_t rl = mkbuf(lo, UPDATE ? 6u * B8 : 0u);
  // the sensor blocks are requested FIRST: they are the only loads of the step that are never cache-resident (a new block
  // every message) and returns are in order per wave (k_step_quad: 43.5 -> 39.8 us at 64k x 21 states with long streams)
  double gyro[3], accel[3], dt, z[3], rd[3];
  bool upd = false;
  if constexpr (UPDATE) upd = (mask == nullptr) || (mask[b] != 0);
  if (bc.on & 1) {  // one IMU message for every filter: kernel arguments (wave-uniform branch)
#pragma unroll
    for (int i = 0; i < 3; i++) { gyro[i] = bc.imu[i]; accel[i] = bc.imu[3 + i]; }
    dt = bc.imu[6];
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      gyro[i] = ldg(ri, i * B8, bo);
      accel[i] = ldg(ri, (3 + i) * B8, bo);
    }
    dt = ldg(ri, 6u * B8, bo);
  }
  if (bc.on & 2) {
#pragma unroll
    for (int i = 0; i < 3; i++) { z[i] = bc.lo[i]; rd[i] = bc.lo[3 + i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      z[i] = UPDATE ? ldg(rl, i * B8, bo) : 0.0;
      rd[i] = UPDATE ? ldg(rl, (3 + i) * B8, bo) : 1.0;
    }
  }
  if (k.qblk != nullptr) {  // per-filter process noise (wave-uniform branch)
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
    qg = ldg(rq, 0u, bo); qa = ldg(rq, B8, bo); qbg = ldg(rq, 2u * B8, bo); qba = ldg(rq, 3u * B8, bo);
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
  imu_process_step<NS>(x, q, P, gyro, accel, dt, qg, qa, qbg, qba, k);
  if constexpr (UPDATE) {
    // Predicated, not branched: lanes whose handler returned NULL (mask 0) run the same stream with D^-1 = 0 and a
    // benign R, so the wave stores whole rows (see measurement_update).
    double resid[3], S[6];
#pragma unroll
    for (int i = 0; i < 3; i++) resid[i] = upd ? z[i] - x[3 + i] : 0.0;  // rbis.cpp:170
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j <= i; j++)
        S[pk(i, j)] = P[pk(3 + i, 3 + j)] + (i == j ? (upd ? rd[i] : 1.0) : 0.0);  // rbis.cpp:134-135
    measurement_update<NS, 3>(x, q, P, ll, resid, S, IdxVel{}, k, [&io](int pi, double v) { io.st(L::OFF_P + pi, v); }, upd);
  } else {
#pragma unroll
    for (int i = 0; i < L::NP; i++) io.st(L::OFF_P + i, P[i]);
  }
#pragma unroll
  for (int i = 0; i < NS; i++) io.st(L::OFF_VEC + i, x[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) io.st(L::OFF_QUAT + i, q[i]);
  io.st(L::OFF_LL, ll);
}

// Two-wave cooperative step (rbis_coop.hpp): 128-thread workgroups, wave 0 = role C (dynamic core sub-matrix, state,
// quaternion), wave 1 = role P (passive omega/accel panels) for the SAME 64 filters = one tile; each role owns a
// contiguous range of the tile's rows (Slots<NS>::ROW_SPLIT); one LDS hand-off + one barrier.
// This is the 21-state hot kernel (231 packed entries do not fit one lane) and the default mapping for n = 15.
// No lane returns before the barrier: lanes past the batch end work on the zero-initialised padding filters of the
// last tile and on bounds-checked (zero) inputs.
template <int NS, bool UPDATE, int MH = MH_DEFAULT, class CORR = NoCorr, bool PREDICT = true>
__global__ __launch_bounds__(128, 1) void k_step_coop(const double *st, double *sto, int B,
                                                      const double *__restrict__ imu, const double *__restrict__ lo,
                                                      const uint8_t *__restrict__ mask, double qg, double qa,
                                                      double qbg, double qba, Consts k, CorrArgs ca, StepBcast bc = StepBcast())
{
  __shared__ double xch[(UPDATE || CORR::M > 0) ? CoopX<NS, CORR>::NXCH : 1][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  // half tiles (Consts::half_tiles, batches that leave workgroup slots empty): workgroup 2 t takes filters 0-31 of tile t, 2 t + 1
  // filters 32-63; lanes l and l + 32 mirror each other, so nothing else in the kernel knows
  const unsigned wgi = xcd_workgroup(k);
  const unsigned tile = k.half_tiles ? (wgi >> 1) : wgi;
  const unsigned lane = k.half_tiles ? ((threadIdx.x & 31u) | ((wgi & 1u) << 5)) : (threadIdx.x & 63u);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA, true> io(st, sto, tile, lane);
  const rsrc_t ri = mkbuf(imu, PREDICT ? 7u * B8 : 0u);
  const rsrc_t rl = mkbuf(lo, UPDATE ? 6u * B8 : 0u);
  StepInputs in;
  if (PREDICT && (bc.on & 1)) {  // one IMU message for every filter: kernel arguments (wave-uniform branch)
#pragma unroll
    for (int i = 0; i < 3; i++) { in.gyro[i] = bc.imu[i]; in.accel[i] = bc.imu[3 + i]; }
    in.dt = bc.imu[6];
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      in.gyro[i] = PREDICT ? ldg(ri, i * B8, bo) : 0.0;
      in.accel[i] = PREDICT ? ldg(ri, (3 + i) * B8, bo) : 0.0;
    }
    in.dt = PREDICT ? ldg(ri, 6u * B8, bo) : 0.0;
  }
  if (PREDICT && (bc.on & 2)) {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.z[i] = bc.lo[i]; in.rd[i] = bc.lo[3 + i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      in.z[i] = UPDATE ? ldg(rl, i * B8, bo) : 0.0;
      in.rd[i] = UPDATE ? ldg(rl, (3 + i) * B8, bo) : 1.0;
    }
  }
  in.upd = UPDATE && (b < (unsigned) B) && (mask == nullptr || mask[b] != 0);
  in.qg = qg; in.qa = qa; in.qbg = qbg; in.qba = qba;
  if (PREDICT && k.qblk != nullptr) {  // per-filter process noise (wave-uniform branch)
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
    in.qg = ldg(rq, 0u, bo); in.qa = ldg(rq, B8, bo); in.qbg = ldg(rq, 2u * B8, bo); in.qba = ldg(rq, 3u * B8, bo);
  }
  CorrInputs cin;
  if constexpr (CORR::M > 0) {
    const rsrc_t rz = mkbuf(ca.z2, (unsigned) CORR::M * B8);
    const rsrc_t rr = mkbuf(ca.r2, ca.r2 ? (unsigned) CORR::M * B8 : 0u);
    const rsrc_t rq2 = mkbuf(ca.qm2, CORR::ORIENT ? 4u * B8 : 0u);
#pragma unroll
    for (int i = 0; i < CORR::M; i++) {
      cin.z[i] = ca.zbc ? ca.zb2[i] : ldg(rz, i * B8, bo);
      cin.rd[i] = ca.r2 ? ldg(rr, i * B8, bo) : ca.rb2[i];
    }
    if (ca.rfull != nullptr) {  // full R (wave-uniform branch): diagonal + strictly-lower part
      const rsrc_t rf = mkbuf(ca.rfull, (unsigned) (CORR::M * CORR::M) * B8);
#pragma unroll
      for (int i = 0; i < CORR::M; i++) {
        cin.rd[i] = ldg(rf, (unsigned) (i * CORR::M + i) * B8, bo);
#pragma unroll
        for (int j = 0; j < i; j++) cin.ro[i * (i - 1) / 2 + j] = ldg(rf, (unsigned) (j * CORR::M + i) * B8, bo);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) cin.qm[i] = CORR::ORIENT ? (ca.zbc ? ca.qb2[i] : ldg(rq2, i * B8, bo)) : 0.0;
    cin.upd = (b < (unsigned) B) && (ca.mask2 == nullptr || ca.mask2[b] != 0);
    // A stand-alone update that NO filter of this tile takes, working in place: nothing to load, nothing to store.  (Both waves
    // of the tile read the same 64 mask bytes, so they leave together -- no barrier is left waiting.)  This is what makes the
    // per-filter choice between two updates (RBISEitherUpdate: LegOdoCommon's pos_and_lin_rate / lin_rate fall-back) cost one
    // state round trip, not two: the half no filter takes returns at once.
    if constexpr (!PREDICT && !UPDATE) {
      if (st == sto && ca.mask2 != nullptr && __ballot(cin.upd) == 0ull) return;
    }
  }
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  if (role == 0) {
    io.template need<0, Slots<NS>::ROW_SPLIT>();
    coop_role_core<NS, UPDATE, CORR, PREDICT>(ld, stf, [lane](int s, double v) { xch[s][lane] = v; }, xrd, sync, in, k, cin);
  } else {
    io.template need<Slots<NS>::ROW_SPLIT, Slots<NS>::NROW>();
    coop_role_passive<NS, UPDATE, CORR, PREDICT>(ld, stf, xrd, sync, in, k, cin);
  }
}

// A role's rows of the predicted posterior into a second tile (k_step_coop_pred, k_step_quad_pred): the role bodies' SP functor.
template <class IO>
struct PredStore {
  static constexpr bool on = true;
  IO *io;
  __device__ __forceinline__ void operator()(int comp, double v) const { io->st(comp, v); }
};

// k_step_coop<NS, true> (plain fused step) that also writes the PREDICTED posterior -- the INS update's, before the leg-odometry
// update behind it: what k_step_coop<NS, false> alone leaves -- into `pred`, a checkpoint slot of the same tiled layout
// (pb_set_pred_slot).  Each role stores its own rows of it the moment its predict is final (SP, rbis_coop.hpp) and goes on with the
// update; the filtered posterior is the same arithmetic, bit for bit.  A kernel of its own rather than a flag of k_step_coop, so
// that every launch without a predicted slot runs the code object it ran before; same inputs, same input order.
template <int NS, int MH = MH_DEFAULT>
__global__ __launch_bounds__(128, 1) void k_step_coop_pred(const double *st, double *sto, double *pred, int B,
                                                           const double *__restrict__ imu, const double *__restrict__ lo,
                                                           const uint8_t *__restrict__ mask, double qg, double qa,
                                                           double qbg, double qba, Consts k, StepBcast bc)
{
  __shared__ double xch[CoopX<NS, NoCorr>::NXCH][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned wgi = xcd_workgroup(k);   // (half tiles: as k_step_coop)
  const unsigned tile = k.half_tiles ? (wgi >> 1) : wgi;
  const unsigned lane = k.half_tiles ? ((threadIdx.x & 31u) | ((wgi & 1u) << 5)) : (threadIdx.x & 63u);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  using IO = TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA, true>;
  IO io(st, sto, tile, lane);
  IO po(pred, pred, tile, lane);   // (only its stores are used)
  const rsrc_t ri = mkbuf(imu, 7u * B8);
  const rsrc_t rl = mkbuf(lo, 6u * B8);
  StepInputs in;
  if (bc.on & 1) {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.gyro[i] = bc.imu[i]; in.accel[i] = bc.imu[3 + i]; }
    in.dt = bc.imu[6];
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.gyro[i] = ldg(ri, i * B8, bo); in.accel[i] = ldg(ri, (3 + i) * B8, bo); }
    in.dt = ldg(ri, 6u * B8, bo);
  }
  if (bc.on & 2) {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.z[i] = bc.lo[i]; in.rd[i] = bc.lo[3 + i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.z[i] = ldg(rl, i * B8, bo); in.rd[i] = ldg(rl, (3 + i) * B8, bo); }
  }
  in.upd = (b < (unsigned) B) && (mask == nullptr || mask[b] != 0);
  in.qg = qg; in.qa = qa; in.qbg = qbg; in.qba = qba;
  if (k.qblk != nullptr) {
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
    in.qg = ldg(rq, 0u, bo); in.qa = ldg(rq, B8, bo); in.qbg = ldg(rq, 2u * B8, bo); in.qba = ldg(rq, 3u * B8, bo);
  }
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  const PredStore<IO> sp{ &po };
  if (role == 0) {
    io.template need<0, Slots<NS>::ROW_SPLIT>();
    coop_role_core<NS, true, NoCorr, true, false, 0>(ld, stf, [lane](int s, double v) { xch[s][lane] = v; }, xrd, sync, in, k, CorrInputs(), sp);
  } else {
    io.template need<Slots<NS>::ROW_SPLIT, Slots<NS>::NROW>();
    coop_role_passive<NS, true, NoCorr, true>(ld, stf, xrd, sync, in, k, CorrInputs(), sp);
  }
}

// k_step_coop<15, true, MH, CORR> (the fused step with a correction stage: pb_step_legodo_correct) that also writes the PREDICTED
// posterior into `pred`, as k_step_coop_pred does for the plain fused step: each role stores its rows of the INS posterior the moment
// its predict is final and goes on into the leg-odometry update and the correction.  Same inputs, same input order, the same
// arithmetic for the filtered posterior, bit for bit.  15 states only: with 21 the correction stage alone already spills (pb_step.hip).
template <int NS, int MH, class CORR>
__global__ __launch_bounds__(128, 1) void k_step_coop_corr_pred(const double *st, double *sto, double *pred, int B,
                                                                const double *__restrict__ imu, const double *__restrict__ lo,
                                                                const uint8_t *__restrict__ mask, double qg, double qa,
                                                                double qbg, double qba, Consts k, CorrArgs ca, StepBcast bc)
{
  static_assert(NS == 15 && CORR::M > 0, "the 15-state fused step with a correction stage");
  __shared__ double xch[CoopX<NS, CORR>::NXCH][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned wgi = xcd_workgroup(k);   // (half tiles: as k_step_coop)
  const unsigned tile = k.half_tiles ? (wgi >> 1) : wgi;
  const unsigned lane = k.half_tiles ? ((threadIdx.x & 31u) | ((wgi & 1u) << 5)) : (threadIdx.x & 63u);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  using IO = TileIO<NS, MemHint<MH>::LA, MemHint<MH>::SA, true>;
  IO io(st, sto, tile, lane);
  IO po(pred, pred, tile, lane);   // (only its stores are used)
  const rsrc_t ri = mkbuf(imu, 7u * B8);
  const rsrc_t rl = mkbuf(lo, 6u * B8);
  StepInputs in;
  if (bc.on & 1) {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.gyro[i] = bc.imu[i]; in.accel[i] = bc.imu[3 + i]; }
    in.dt = bc.imu[6];
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.gyro[i] = ldg(ri, i * B8, bo); in.accel[i] = ldg(ri, (3 + i) * B8, bo); }
    in.dt = ldg(ri, 6u * B8, bo);
  }
  if (bc.on & 2) {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.z[i] = bc.lo[i]; in.rd[i] = bc.lo[3 + i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) { in.z[i] = ldg(rl, i * B8, bo); in.rd[i] = ldg(rl, (3 + i) * B8, bo); }
  }
  in.upd = (b < (unsigned) B) && (mask == nullptr || mask[b] != 0);
  in.qg = qg; in.qa = qa; in.qbg = qbg; in.qba = qba;
  if (k.qblk != nullptr) {
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
    in.qg = ldg(rq, 0u, bo); in.qa = ldg(rq, B8, bo); in.qbg = ldg(rq, 2u * B8, bo); in.qba = ldg(rq, 3u * B8, bo);
  }
  CorrInputs cin;   // (as k_step_coop)
  const rsrc_t rz = mkbuf(ca.z2, (unsigned) CORR::M * B8);
  const rsrc_t rr = mkbuf(ca.r2, ca.r2 ? (unsigned) CORR::M * B8 : 0u);
  const rsrc_t rq2 = mkbuf(ca.qm2, CORR::ORIENT ? 4u * B8 : 0u);
#pragma unroll
  for (int i = 0; i < CORR::M; i++) {
    cin.z[i] = ca.zbc ? ca.zb2[i] : ldg(rz, i * B8, bo);
    cin.rd[i] = ca.r2 ? ldg(rr, i * B8, bo) : ca.rb2[i];
  }
  if (ca.rfull != nullptr) {
    const rsrc_t rf = mkbuf(ca.rfull, (unsigned) (CORR::M * CORR::M) * B8);
#pragma unroll
    for (int i = 0; i < CORR::M; i++) {
      cin.rd[i] = ldg(rf, (unsigned) (i * CORR::M + i) * B8, bo);
#pragma unroll
      for (int j = 0; j < i; j++) cin.ro[i * (i - 1) / 2 + j] = ldg(rf, (unsigned) (j * CORR::M + i) * B8, bo);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) cin.qm[i] = CORR::ORIENT ? (ca.zbc ? ca.qb2[i] : ldg(rq2, i * B8, bo)) : 0.0;
  cin.upd = (b < (unsigned) B) && (ca.mask2 == nullptr || ca.mask2[b] != 0);
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  const PredStore<IO> sp{ &po };
  if (role == 0) {
    io.template need<0, Slots<NS>::ROW_SPLIT>();
    coop_role_core<NS, true, CORR, true, false, 0>(ld, stf, [lane](int s, double v) { xch[s][lane] = v; }, xrd, sync, in, k, cin, sp);
  } else {
    io.template need<Slots<NS>::ROW_SPLIT, Slots<NS>::NROW>();
    coop_role_passive<NS, true, CORR, true>(ld, stf, xrd, sync, in, k, cin, sp);
  }
}

// The 21-state hot step on FOUR cooperating waves per 64 filters (rbis_quad.hpp): <= 256 registers per role, so two
// workgroups (8 waves) share a CU and one tile's loads overlap another's arithmetic and stores.  Same inputs, same
// posterior (to rounding: the c-b coupling enters P_cc as one additive term instead of inside the row operations) and the
// same bytes as k_step_coop<21>.  No lane returns before the barriers (see k_step_coop).
template <bool UPDATE, int MH = MH_DEFAULT>
__global__ __launch_bounds__(256, 2) void k_step_quad(const double *st, double *sto, int B,
                                                      const double *__restrict__ imu, const double *__restrict__ lo,
                                                      const uint8_t *__restrict__ mask, double qg, double qa,
                                                      double qbg, double qba, Consts k, StepBcast bc)
{
  using SL = Slots<21>;
  __shared__ double xch[Quad::NXCH][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<21, MemHint<MH>::LA, MemHint<MH>::SA> io(st, sto, tile, lane);
  // every role fetches its own copy of the inputs INSIDE its branch: nothing but addresses is live across the dispatch
  auto inputs = [&](bool meas) {
    const rsrc_t ri = mkbuf(imu, 7u * B8);
    const rsrc_t rl = mkbuf(lo, UPDATE ? 6u * B8 : 0u);
    StepInputs in;
    if (bc.on & 1) {  // one IMU message for every filter: kernel arguments (wave-uniform branch)
#pragma unroll
      for (int i = 0; i < 3; i++) { in.gyro[i] = bc.imu[i]; in.accel[i] = bc.imu[3 + i]; }
      in.dt = bc.imu[6];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        in.gyro[i] = ldg(ri, i * B8, bo);
        in.accel[i] = ldg(ri, (3 + i) * B8, bo);
      }
      in.dt = ldg(ri, 6u * B8, bo);
    }
    if (bc.on & 2) {
#pragma unroll
      for (int i = 0; i < 3; i++) { in.z[i] = bc.lo[i]; in.rd[i] = bc.lo[3 + i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        in.z[i] = (UPDATE && meas) ? ldg(rl, i * B8, bo) : 0.0;
        in.rd[i] = (UPDATE && meas) ? ldg(rl, (3 + i) * B8, bo) : 1.0;
      }
    }
    in.upd = UPDATE && (b < (unsigned) B) && (mask == nullptr || mask[b] != 0);
    in.qg = qg; in.qa = qa; in.qbg = qbg; in.qba = qba;
    if (k.qblk != nullptr) {  // per-filter process noise (wave-uniform branch)
      const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
      in.qg = ldg(rq, 0u, bo); in.qa = ldg(rq, B8, bo); in.qbg = ldg(rq, 2u * B8, bo); in.qba = ldg(rq, 3u * B8, bo);
    }
    return in;
  };
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  auto xwr = [lane](int s, double v) { xch[s][lane] = v; };
  // the sensor blocks are requested FIRST: they are the only loads of the step that are never cache-resident (a new block
  // every message), and returns are in order per wave
  if (role == 0) {
    const StepInputs in = inputs(true);
    io.template need<SL::QROW[0], SL::QROW[1]>();
    quad_role_cc<UPDATE>(ld, stf, xwr, xrd, sync, in, k);
  } else if (role == 1) {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[1], SL::QROW[2]>();
    quad_role_cb<UPDATE>(ld, stf, xwr, xrd, sync, in, k);
  } else if (role == 2) {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[2], SL::QROW[3]>();
    quad_role_passive<UPDATE, 0, 0, true>(ld, stf, xwr, xrd, sync, in, k);
  } else {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[3], SL::QROW[4]>();
    quad_role_passive<UPDATE, 1, 0, true>(ld, stf, xwr, xrd, sync, in, k);
  }
}

// k_step_quad<true> that also writes the predicted posterior into `pred` (pb_set_pred_slot; see k_step_coop_pred): roles CB, PW, PA
// store their predicted rows in front of barrier A, role CC its P_cc behind it (role CB's terms arrive there).  A kernel of its own
// so that k_step_quad's code object stays what it was; same inputs, same arithmetic, the filtered posterior bit for bit.
template <int MH = MH_DEFAULT>
__global__ __launch_bounds__(256, 2) void k_step_quad_pred(const double *st, double *sto, double *pred, int B,
                                                           const double *__restrict__ imu, const double *__restrict__ lo,
                                                           const uint8_t *__restrict__ mask, double qg, double qa,
                                                           double qbg, double qba, Consts k, StepBcast bc)
{
  using SL = Slots<21>;
  using IO = TileIO<21, MemHint<MH>::LA, MemHint<MH>::SA>;
  __shared__ double xch[Quad::NXCH][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = xcd_workgroup(k);
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  IO io(st, sto, tile, lane);
  IO po(pred, pred, tile, lane);   // (only its stores are used)
  auto inputs = [&](bool meas) {
    const rsrc_t ri = mkbuf(imu, 7u * B8);
    const rsrc_t rl = mkbuf(lo, 6u * B8);
    StepInputs in;
    if (bc.on & 1) {
#pragma unroll
      for (int i = 0; i < 3; i++) { in.gyro[i] = bc.imu[i]; in.accel[i] = bc.imu[3 + i]; }
      in.dt = bc.imu[6];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) { in.gyro[i] = ldg(ri, i * B8, bo); in.accel[i] = ldg(ri, (3 + i) * B8, bo); }
      in.dt = ldg(ri, 6u * B8, bo);
    }
    if (bc.on & 2) {
#pragma unroll
      for (int i = 0; i < 3; i++) { in.z[i] = bc.lo[i]; in.rd[i] = bc.lo[3 + i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) { in.z[i] = meas ? ldg(rl, i * B8, bo) : 0.0; in.rd[i] = meas ? ldg(rl, (3 + i) * B8, bo) : 1.0; }
    }
    in.upd = (b < (unsigned) B) && (mask == nullptr || mask[b] != 0);
    in.qg = qg; in.qa = qa; in.qbg = qbg; in.qba = qba;
    if (k.qblk != nullptr) {
      const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
      in.qg = ldg(rq, 0u, bo); in.qa = ldg(rq, B8, bo); in.qbg = ldg(rq, 2u * B8, bo); in.qba = ldg(rq, 3u * B8, bo);
    }
    return in;
  };
  auto ld = [&io](int comp) { return io.ld(comp); };
  auto stf = [&io](int comp, double v) { io.st(comp, v); };
  auto sync = []() { __syncthreads(); };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  auto xwr = [lane](int s, double v) { xch[s][lane] = v; };
  const PredStore<IO> sp{ &po };
  if (role == 0) {
    const StepInputs in = inputs(true);
    io.template need<SL::QROW[0], SL::QROW[1]>();
    quad_role_cc<true, false, 0, true>(ld, stf, xwr, xrd, sync, in, k, SixIn(), sp);
  } else if (role == 1) {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[1], SL::QROW[2]>();
    quad_role_cb<true, 0>(ld, stf, xwr, xrd, sync, in, k, sp);
  } else if (role == 2) {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[2], SL::QROW[3]>();
    quad_role_passive<true, 0, 0, true>(ld, stf, xwr, xrd, sync, in, k, SixIn(), sp);
  } else {
    const StepInputs in = inputs(false);
    io.template need<SL::QROW[3], SL::QROW[4]>();
    quad_role_passive<true, 1, 0, true>(ld, stf, xwr, xrd, sync, in, k, SixIn(), sp);
  }
}

}  // namespace pb
