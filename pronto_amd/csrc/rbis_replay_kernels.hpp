// rbis_replay_kernels.hpp -- the time-fused replay kernels: T steps per launch with the state resident in registers (k_replay_fused one
// lane per filter, k_replay_coop two waves per tile, k_replay_quad four).  Launched from pb_step.hip (pbk_replay_fused).
// Tile I/O and argument structs: rbis_tile_io.hpp.
#pragma once

#include "rbis_tile_io.hpp"
#include "rbis_coop.hpp"
#include "rbis_quad.hpp"

namespace pb {

// Time-fused replay: T consecutive predict+update steps per launch with the state and P resident in registers; only the
// 104 B/filter of inputs stream from HBM per step, the posterior is materialised once per launch.  This is NOT the plugin
// path (MavStateEstimator::addUpdate publishes a posterior per message) but what a parameter sweep or a likelihood
// evaluation over a log segment wants (param_sweep.py:39-52).  Accounting: 104 + 2240/T bytes per filter-step, so the
// bound moves from HBM to fp64 VALU issue; bench.py reports it separately (never as the headline value).
// Each step requests its inputs at its top.
template <int NS>
__global__ __launch_bounds__(64, 1) void k_replay_fused(double *__restrict__ st, int B, int T,
                                                        const double *__restrict__ imu, const double *__restrict__ lo,
                                                        const uint8_t *__restrict__ mask, double qg, double qa, double qbg,
                                                        double qba, Consts k)
{
  using L = Lay<NS>;
  const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (unsigned) B) return;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, 0, 0> io(st, st, blockIdx.x, threadIdx.x);
  io.template need<0, Slots<NS>::NROW>();
  double x[NS], q[4], ll, P[L::NP];
#pragma unroll
  for (int i = 0; i < NS; i++) x[i] = io.ld(L::OFF_VEC + i);
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = io.ld(L::OFF_QUAT + i);
  ll = io.ld(L::OFF_LL);
#pragma unroll
  for (int i = 0; i < L::NP; i++) P[i] = io.ld(L::OFF_P + i);
  if (k.qblk != nullptr) {
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
    qg = ldg(rq, 0u, bo); qa = ldg(rq, B8, bo); qbg = ldg(rq, 2u * B8, bo); qba = ldg(rq, 3u * B8, bo);
  }
  // step-t input blocks are [7][B] / [6][B] / [B] slabs of the streams; 64-bit slab base, 32-bit offsets inside
  double in[13];
  bool upd;
  auto fetch = [&](int t, double (&dst)[13], bool &u) {
    const rsrc_t ri = mkbuf(imu + (size_t) t * 7 * B, 7u * B8);
    const rsrc_t rl = mkbuf(lo + (size_t) t * 6 * B, 6u * B8);
#pragma unroll
    for (int i = 0; i < 7; i++) dst[i] = ldg(ri, i * B8, bo);
#pragma unroll
    for (int i = 0; i < 6; i++) dst[7 + i] = ldg(rl, i * B8, bo);
    u = (mask == nullptr) || (mask[(size_t) t * B + b] != 0);
  };
  fetch(0, in, upd);
  for (int t = 0; t < T; t++) {
    if (t > 0) fetch(t, in, upd);
    const double gyro[3] = { in[0], in[1], in[2] }, accel[3] = { in[3], in[4], in[5] };
    imu_process_step<NS>(x, q, P, gyro, accel, in[6], qg, qa, qbg, qba, k);
    double resid[3], S[6];
#pragma unroll
    for (int i = 0; i < 3; i++) resid[i] = upd ? in[7 + i] - x[3 + i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) S[pk(i, j)] = P[pk(3 + i, 3 + j)] + (i == j ? (upd ? in[10 + i] : 1.0) : 0.0);
    measurement_update<NS, 3>(x, q, P, ll, resid, S, IdxVel{}, k, NoSink(), upd);
  }
#pragma unroll
  for (int i = 0; i < L::NP; i++) io.st(L::OFF_P + i, P[i]);
#pragma unroll
  for (int i = 0; i < NS; i++) io.st(L::OFF_VEC + i, x[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) io.st(L::OFF_QUAT + i, q[i]);
  io.st(L::OFF_LL, ll);
}

// Time-fused replay on the cooperative mapping: T consecutive predict + leg-odometry steps per launch with each role's part
// of the state resident in ITS registers; only the 104 B/filter of inputs stream from HBM per step and the posterior is
// written once per launch.  Per step the two roles trade what the other needs of the state vector through LDS (role C
// gives v chi Delta [biases] quat, role P gives omega accel: the process blocks linearise about the whole prior state),
// then run exactly the bodies of k_step_coop with loads and stores redirected to registers.  Two barriers per step.
// No per-message posterior: NOT the plugin path (see pb_replay_legodo_fused); accounting 104 + 2*state/T bytes per step.
template <int NS>
__global__ __launch_bounds__(128, 1) void k_replay_coop(double *st, int B, int T, const double *__restrict__ imu,
                                                        const double *__restrict__ lo, const uint8_t *__restrict__ mask,
                                                        double qg, double qa, double qbg, double qba, Consts k, SlotOut so)
{
  using L = Lay<NS>;
  using C = Coop<NS>;
  using SL = Slots<NS>;
  __shared__ double xch[C::NXCH][64];
  __shared__ double xst[NS + 4][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = blockIdx.x;
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, 0, 0, true> io(st, st, tile, lane);
  double q4[4] = { qg, qa, qbg, qba };
  if (k.qblk != nullptr) {
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
#pragma unroll
    for (int i = 0; i < 4; i++) q4[i] = ldg(rq, (unsigned) i * B8, bo);
  }
  auto sync = []() { __syncthreads(); };
  auto xw = [lane](int s, double v) { xch[s][lane] = v; };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  // inputs of step t (both roles need the IMU block; role C the measurement)
  auto inputs = [&](int t) {
    const rsrc_t ri = mkbuf(imu + (size_t) t * 7 * B, 7u * B8);
    const rsrc_t rl = mkbuf(lo + (size_t) t * 6 * B, 6u * B8);
    StepInputs in;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      in.gyro[i] = ldg(ri, i * B8, bo);
      in.accel[i] = ldg(ri, (3 + i) * B8, bo);
      in.z[i] = ldg(rl, i * B8, bo);
      in.rd[i] = ldg(rl, (3 + i) * B8, bo);
    }
    in.dt = ldg(ri, 6u * B8, bo);
    in.upd = (b < (unsigned) B) && (mask == nullptr || mask[(size_t) t * B + b] != 0);
    in.qg = q4[0]; in.qa = q4[1]; in.qbg = q4[2]; in.qba = q4[3];
    return in;
  };
  // The two roles run SEPARATE loops (the same two barriers per iteration in each): with one loop around a role branch
  // every component of both roles would be live across the back edge.
  if (role == 0) {
    double V[L::NC];  // canonical components; a role only ever touches its own ones plus the other's state vector
    io.template need<0, SL::ROW_SPLIT>();
    static_for<SL::NSLOT>([&](auto I) {
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
      if constexpr (comp >= 0 && SL::T.role2[slot] == 0) V[comp] = io.ld(comp);
    });
    auto ld = [&V](int comp) { return V[comp]; };
    auto stf = [&V](int comp, double v) { V[comp] = v; };
    for (int t = 0; t < T; t++) {
      const StepInputs in = inputs(t);
#pragma unroll
      for (int i = 0; i < C::NSC; i++) xst[C::fullc(i)][lane] = V[L::OFF_VEC + C::fullc(i)];
#pragma unroll
      for (int i = 0; i < 4; i++) xst[NS + i][lane] = V[L::OFF_QUAT + i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 6; i++) V[L::OFF_VEC + C::fullp(i)] = xst[C::fullp(i)][lane];
      coop_role_core<NS, true>(ld, stf, xw, xrd, sync, in, k);
      // (no third barrier: this role overwrites the hand-off only behind the next state-exchange barrier, which role P
      // reaches after it has finished reading; the exchange slots of the two roles are disjoint)
      if (so.base != nullptr) {  // write-through: this role's components of the posterior of step t
        TileIO<NS, 0, MemHint<MH_STREAM_NT>::SA, true> ios(st, so.base + (size_t) t * so.stride, tile, lane);
        static_for<SL::NSLOT>([&](auto I) {
          constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
          if constexpr (comp >= 0 && SL::T.role2[slot] == 0) ios.st(comp, V[comp]);
        });
      }
    }
    static_for<SL::NSLOT>([&](auto I) {
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
      if constexpr (comp >= 0 && SL::T.role2[slot] == 0) io.st(comp, V[comp]);
    });
  } else {
    double V[L::NC];
    io.template need<SL::ROW_SPLIT, SL::NROW>();
    static_for<SL::NSLOT>([&](auto I) {
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
      if constexpr (comp >= 0 && SL::T.role2[slot] == 1) V[comp] = io.ld(comp);
    });
    auto ld = [&V](int comp) { return V[comp]; };
    auto stf = [&V](int comp, double v) { V[comp] = v; };
    for (int t = 0; t < T; t++) {
      const StepInputs in = inputs(t);
#pragma unroll
      for (int i = 0; i < 6; i++) xst[C::fullp(i)][lane] = V[L::OFF_VEC + C::fullp(i)];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < C::NSC; i++) V[L::OFF_VEC + C::fullc(i)] = xst[C::fullc(i)][lane];
#pragma unroll
      for (int i = 0; i < 4; i++) V[L::OFF_QUAT + i] = xst[NS + i][lane];
      coop_role_passive<NS, true>(ld, stf, xrd, sync, in, k);
      if (so.base != nullptr) {
        TileIO<NS, 0, MemHint<MH_STREAM_NT>::SA, true> ios(st, so.base + (size_t) t * so.stride, tile, lane);
        static_for<SL::NSLOT>([&](auto I) {
          constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
          if constexpr (comp >= 0 && SL::T.role2[slot] == 1) ios.st(comp, V[comp]);
        });
      }
    }
    static_for<SL::NSLOT>([&](auto I) {
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];
      if constexpr (comp >= 0 && SL::T.role2[slot] == 1) io.st(comp, V[comp]);
    });
  }
}

// Time-fused replay of a 21-state batch on the FOUR-wave mapping: each role keeps the components it owns (Slots<21>::QROW
// row ranges) in ITS registers for T steps and runs the bodies of k_step_quad with loads and stores redirected to them.  Per
// step the owners of the state vector trade it through LDS (role PW: v chi Delta quat; role CB: biases, omega; role PA:
// accel -- every role linearises about the whole prior state), three barriers per step; the next step's sensor block is
// requested before this step's arithmetic.  OCC = waves per SIMD the register budget is cut for (2: 256 registers per role
// and 452 B of scratch, two workgroups per CU; 1: no scratch, one workgroup per CU: the faster one, see pb_step.hip).
template <int OCC>
__global__ __launch_bounds__(256, OCC) void k_replay_quad(double *st, int B, int T, const double *__restrict__ imu,
                                                        const double *__restrict__ lo, const uint8_t *__restrict__ mask,
                                                        double qg, double qa, double qbg, double qba, Consts k, SlotOut so)
{
  constexpr int NS = 21;
  using L = Lay<NS>;
  using SL = Slots<NS>;
  __shared__ double xch[Quad::NXCH][64];
  __shared__ double xst[NS + 4][64];
  const int role = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = blockIdx.x;
  const unsigned b = tile * 64u + lane;
  const unsigned bo = b * 8u, B8 = (unsigned) B * 8u;
  TileIO<NS, 0, 0> io(st, st, tile, lane);
  double q4[4] = { qg, qa, qbg, qba };
  if (k.qblk != nullptr) {
    const rsrc_t rq = mkbuf(k.qblk, 4u * B8);
#pragma unroll
    for (int i = 0; i < 4; i++) q4[i] = ldg(rq, (unsigned) i * B8, bo);
  }
  auto sync = []() { __syncthreads(); };
  auto xw = [lane](int s, double v) { xch[s][lane] = v; };
  auto xrd = [lane](int s) { return xch[s][lane]; };
  auto inputs = [&](int t, bool meas) {
    const rsrc_t ri = mkbuf(imu + (size_t) t * 7 * B, 7u * B8);
    const rsrc_t rl = mkbuf(lo + (size_t) t * 6 * B, 6u * B8);
    StepInputs in;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      in.gyro[i] = ldg(ri, i * B8, bo);
      in.accel[i] = ldg(ri, (3 + i) * B8, bo);
      in.z[i] = meas ? ldg(rl, i * B8, bo) : 0.0;
      in.rd[i] = meas ? ldg(rl, (3 + i) * B8, bo) : 1.0;
    }
    in.dt = ldg(ri, 6u * B8, bo);
    in.upd = (b < (unsigned) B) && (mask == nullptr || mask[(size_t) t * B + b] != 0);
    in.qg = q4[0]; in.qa = q4[1]; in.qbg = q4[2]; in.qba = q4[3];
    return in;
  };
  // state-vector slots of xst: x[i] at i, quat at NS + i.  Owner of each entry in the four-wave mapping:
  //   role 1 (CB): x[0..2] omega, x[15..20] biases;  role 2 (PW): x[3..11] v chi Delta, quat;  role 3 (PA): x[12..14] accel
  // The four roles run SEPARATE loops (the same three barriers per iteration in each), see k_replay_coop.
#define PB_REPLAY_QUAD_ROLE(ROLE_ID, MEAS, OWN_EXPR, BODY)                                                            \
  {                                                                                                                   \
    double V[L::NC];                                                                                                  \
    io.template need<SL::QROW[ROLE_ID], SL::QROW[ROLE_ID + 1]>();                                                     \
    static_for<SL::NSLOT>([&](auto I) {                                                                               \
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];                                            \
      if constexpr (comp >= 0 && slot >= SL::T.nq[ROLE_ID] - (SL::QROW[ROLE_ID + 1] - SL::QROW[ROLE_ID]) * 2 &&       \
                    slot < SL::T.nq[ROLE_ID])                                                                         \
        V[comp] = io.ld(comp);                                                                                        \
    });                                                                                                               \
    auto ld = [&V](int comp) { return V[comp]; };                                                                     \
    auto stf = [&V](int comp, double v) { V[comp] = v; };                                                             \
    auto own = [](int i) { return OWN_EXPR; };                                                                        \
    StepInputs nxt = inputs(0, MEAS);                                                                                 \
    for (int t = 0; t < T; t++) {                                                                                     \
      const StepInputs in = nxt;                                                                                      \
      if (t + 1 < T) nxt = inputs(t + 1, MEAS);                                                                       \
      static_for<NS + 4>([&](auto I) {                                                                                \
        constexpr int i = decltype(I)::value;                                                                         \
        if (own(i)) xst[i][lane] = V[i < NS ? L::OFF_VEC + i : L::OFF_QUAT + (i - NS)];                               \
      });                                                                                                             \
      __syncthreads();                                                                                                \
      static_for<NS + 4>([&](auto I) {                                                                                \
        constexpr int i = decltype(I)::value;                                                                         \
        if (!own(i)) V[i < NS ? L::OFF_VEC + i : L::OFF_QUAT + (i - NS)] = xst[i][lane];                              \
      });                                                                                                             \
      BODY;                                                                                                           \
      if (so.base != nullptr) { /* write-through: this role's rows of the posterior of step t */                      \
        TileIO<NS, 0, MemHint<MH_STREAM_NT>::SA> ios(st, so.base + (size_t) t * so.stride, tile, lane);               \
        static_for<SL::NSLOT>([&](auto I) {                                                                           \
          constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];                                        \
          if constexpr (comp >= 0 && slot >= SL::T.nq[ROLE_ID] - (SL::QROW[ROLE_ID + 1] - SL::QROW[ROLE_ID]) * 2 &&   \
                        slot < SL::T.nq[ROLE_ID])                                                                     \
            ios.st(comp, V[comp]);                                                                                    \
        });                                                                                                           \
      }                                                                                                               \
    }                                                                                                                 \
    static_for<SL::NSLOT>([&](auto I) {                                                                               \
      constexpr int slot = decltype(I)::value, comp = SL::T.comp_of[slot];                                            \
      if constexpr (comp >= 0 && slot >= SL::T.nq[ROLE_ID] - (SL::QROW[ROLE_ID + 1] - SL::QROW[ROLE_ID]) * 2 &&       \
                    slot < SL::T.nq[ROLE_ID])                                                                         \
        io.st(comp, V[comp]);                                                                                         \
    });                                                                                                               \
  }
  if (role == 0) PB_REPLAY_QUAD_ROLE(0, true, false, (quad_role_cc<true, false, 0, false>(ld, stf, xw, xrd, sync, in, k)))
  else if (role == 1) PB_REPLAY_QUAD_ROLE(1, false, (i < 3 || (i >= 15 && i < NS)), (quad_role_cb<true>(ld, stf, xw, xrd, sync, in, k)))
  else if (role == 2) PB_REPLAY_QUAD_ROLE(2, false, ((i >= 3 && i < 12) || i >= NS), (quad_role_passive<true, 0>(ld, stf, xw, xrd, sync, in, k)))
  else PB_REPLAY_QUAD_ROLE(3, false, (i >= 12 && i < 15), (quad_role_passive<true, 1>(ld, stf, xw, xrd, sync, in, k)))
#undef PB_REPLAY_QUAD_ROLE
}

}  // namespace pb
